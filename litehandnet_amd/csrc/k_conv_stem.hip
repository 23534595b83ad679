// The stem convolution: dense k x k on the 3-channel NCHW image, NHWC fp32 output (lhn_conv_stem_fwd / lhn_conv_stem_bwd).
// A direct kernel for any k and Cout, MFMA kernels for the two stems the models use (3x3 -> 32, 7x7 -> 64); the epilogue
// accumulates this layer's BatchNorm statistics.  (k_stem.hip is something else: the fused inference stem tail.)
#include "lhn_common.h"

// ------------------------------------------------------------------ stem forward (NCHW 3-channel image -> NHWC)
// thread = (output pixel, group of 8 output channels).  Cout = 40 (mynet at width 160) has five groups: 51 pixel lanes, and thread
// 255 is left over -- it takes no pixel and only joins the barriers.
__global__ void __launch_bounds__(256) k_stem_fwd(const float* __restrict__ img, const float* __restrict__ w, lhn_view y,
                                                  double* __restrict__ stats, int Hi, int Wi, int K, int stride, int pad,
                                                  lhn_bnfin fin) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int CO = y.C, CG = CO >> 3, KK = K * K, T = 3 * KK;
  float* Ws = smem;                                  // [T][CO]
  float* red = smem + T * CO;                        // [256][16]
  const int tid = threadIdx.x;
  for (int i = tid; i < T * CO; i += 256) {
    const int co = i / T, t = i - co * T;
    Ws[t * CO + co] = w[i];
  }
  __syncthreads();
  const int cg = tid % CG, pl = tid / CG, PL = 256 / CG;
  const int64_t total = (int64_t)y.N * y.H * y.W;
  float s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
  for (int64_t pix = pl < PL ? (int64_t)blockIdx.x * PL + pl : total; pix < total; pix += (int64_t)gridDim.x * PL) {
    const int wo = (int)(pix % y.W);
    const int64_t t = pix / y.W;
    const int ho = (int)(t % y.H), n = (int)(t / y.H);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int c = 0; c < 3; ++c) {
      const float* plane = img + ((int64_t)n * 3 + c) * Hi * Wi;
      for (int kh = 0; kh < K; ++kh) {
        const int ih = ho * stride - pad + kh;
        if (ih < 0 || ih >= Hi) continue;
        for (int kw = 0; kw < K; ++kw) {
          const int iw = wo * stride - pad + kw;
          if (iw < 0 || iw >= Wi) continue;
          const float v = plane[(int64_t)ih * Wi + iw];
          const float* wr = Ws + (c * KK + kh * K + kw) * CO + cg * 8;
          const f4 w0 = *reinterpret_cast<const f4*>(wr), w1 = *reinterpret_cast<const f4*>(wr + 4);
          acc[0] += v * w0.x; acc[1] += v * w0.y; acc[2] += v * w0.z; acc[3] += v * w0.w;
          acc[4] += v * w1.x; acc[5] += v * w1.y; acc[6] += v * w1.z; acc[7] += v * w1.w;
        }
      }
    }
    float* o = y.data + pix * y.cstride + y.coff + cg * 8;
    *reinterpret_cast<f4*>(o) = (f4){acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f4*>(o + 4) = (f4){acc[4], acc[5], acc[6], acc[7]};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s[j] += acc[j];
      q[j] += acc[j] * acc[j];
    }
  }
  if (stats) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[tid * 16 + j] = s[j];
      red[tid * 16 + 8 + j] = q[j];
    }
    __syncthreads();
    if (tid < CO) {
      const int g = tid >> 3, j = tid & 7;
      double sd = 0, qd = 0;
      for (int p = 0; p < PL; ++p) {
        sd += red[(p * CG + g) * 16 + j];
        qd += red[(p * CG + g) * 16 + 8 + j];
      }
      double* st = stats + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * CO;
      atomicAdd(st + tid, sd);
      atomicAdd(st + CO + tid, qd);
    }
    if (fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block(fin, stats);
  }
}


// ------------------------------------------------------------------ stem forward, 3x3 -> 32 features (the stems of
// litehourglass.py / liteHandNet.py / lite_hrnet.py) on MFMA: out[pixel][co] = patch[pixel][27 taps] * W^T is a GEMM with
// K = 27 (padded to 32).  The block parks the im2col patch of a 256-pixel tile in LDS (thread = pixel: its 27 image taps are
// loaded ONCE; the direct kernel k_stem_fwd re-reads them per group of 8 features and is bound by 216 LDS weight reads per
// pixel: 125 us for a 184 MB problem); every wave holds all weights as 16 MFMA B registers and runs 2 x 16
// v_mfma_f32_32x32x2_f32 over its 64 pixels.  The accumulator layout gives each lane ONE feature: stores are 128-byte rows,
// statistics need no cross-lane work beyond the two lane halves.  The next tile's taps are loaded while this one computes.
__global__ void __launch_bounds__(256) k_stem3_fwd_mfma(const float* __restrict__ img, const float* __restrict__ w, lhn_view y,
                                                        double* __restrict__ stats, int Hi, int Wi, int stride, int pad, lhn_bnfin fin) {
  constexpr int CO = 32, LDV = 36;
  __shared__ __attribute__((aligned(16))) float Vs[256 * LDV];      // [pixel][tap], columns 27..31 stay zero
  __shared__ double redd[4][2 * CO];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  // B fragments: MFMA step ks, lane (n = l31, k = lh) holds W[tap = 16 lh + ks][co = l31]  (the A reads use the same K order)
  float wreg[16];
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const int tap = 16 * lh + ks;
    wreg[ks] = tap < 27 ? w[l31 * 27 + tap] : 0.f;
  }
  for (int t = 27; t < 32; ++t) Vs[tid * LDV + t] = 0.f;
  const int64_t total = (int64_t)y.N * y.H * y.W;
  const int64_t ntiles = (total + 255) / 256;
  float v[27];
  auto issue = [&](int64_t tile) __attribute__((always_inline)) {
    const int64_t pix = tile * 256 + tid;
    const int64_t pc = pix < total ? pix : total - 1;
    const int wo = (int)(pc % y.W);
    const int64_t r = pc / y.W;
    const int ho = (int)(r % y.H), n = (int)(r / y.H);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* plane = img + ((int64_t)n * 3 + c) * Hi * Wi;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int ih = ho * stride - pad + kh, ihc = min(max(ih, 0), Hi - 1);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int iw = wo * stride - pad + kw, iwc = min(max(iw, 0), Wi - 1);
          const float t = plane[(int64_t)ihc * Wi + iwc];
          v[c * 9 + kh * 3 + kw] = (ih == ihc && iw == iwc) ? t : 0.f;
        }
      }
    }
  };
  float s = 0.f, q = 0.f, kk = 0.f;      // this lane's feature: shifted sums over its pixels (see TileStat)
  int cnt = 0;
  int64_t tile = blockIdx.x;
  if (tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();                       // the previous tile's A reads are done
#pragma unroll
    for (int t = 0; t < 27; ++t) Vs[tid * LDV + t] = v[t];
    __syncthreads();
    if (tile + gridDim.x < ntiles) issue(tile + gridDim.x);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int prow = wave * 64 + 32 * h;
      const f4* ap = reinterpret_cast<const f4*>(Vs + (prow + l31) * LDV + 16 * lh);
      const f4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3];
      const float a[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
      f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks], wreg[ks], acc, 0, 0, 0);
      const int64_t pbase = tile * 256 + prow + 4 * lh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t pix = pbase + (r & 3) + 8 * (r >> 2);
        if (pix < total) {
          y.data[pix * y.cstride + y.coff + l31] = acc[r];
          if (cnt == 0) kk = acc[r];
          const float d = acc[r] - kk;
          s += d;
          q += d * d;
          ++cnt;
        }
      }
    }
  }
  if (stats) {
    const double k0 = kk, c0 = cnt;
    double sd = (double)s + c0 * k0, qd = (double)q + 2.0 * k0 * (double)s + c0 * k0 * k0;
    sd += __shfl_xor(sd, 32, 64);
    qd += __shfl_xor(qd, 32, 64);
    if (lh == 0) {
      redd[wave][l31] = sd;
      redd[wave][CO + l31] = qd;
    }
    __syncthreads();
    if (tid < 2 * CO) {
      double* st = stats + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * CO;
      atomicAdd(st + tid, redd[0][tid] + redd[1][tid] + redd[2][tid] + redd[3][tid]);
    }
    if (fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block(fin, stats);
  }
}


// ------------------------------------------------------------------ stem forward, 7x7 -> 64 features (hourglassnet.py:96) on MFMA
// K = 147 taps padded to 160.  64-pixel tiles (42 KB of LDS: 3 blocks per CU); wave = (32-pixel group, 32-feature tile), its
// weights are 80 MFMA B registers.  thread = (pixel, one of 4 tap groups) loads 37 taps; the next tile's are prefetched.
// The direct kernel took 1.9 ms for this layer at batch 64 (147 x 8 scalar FMAs and 2 LDS reads per tap and thread).
__global__ void __launch_bounds__(256, 2) k_stem7_fwd_mfma(const float* __restrict__ img, const float* __restrict__ w, lhn_view y,
                                                        double* __restrict__ stats, int Hi, int Wi, int stride, int pad, lhn_bnfin fin) {
  constexpr int CO = 64, T = 147, TP = 160, NKS = TP / 2, LDV = TP + 4, BMP = 64, G = 4, NR = 6, NV = NR * 7;      // thread = (pixel, tap-row group): rows (c, kh) g, g+4, .. of 21, 7 kw each
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Vs = smem;                                   // [BMP][LDV], columns 147..159 stay zero
  double* redd = reinterpret_cast<double*>(smem + BMP * LDV);      // [2 pixel groups][2 * CO]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int cot = wave & 1, pg = wave >> 1, co = cot * 32 + l31;
  float wreg[NKS];                                    // step ks, lane (n = l31, k = lh): W[co][tap = NKS * lh + ks]
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int tap = NKS * lh + ks;
    wreg[ks] = tap < T ? w[co * T + tap] : 0.f;
  }
  const int p = tid & (BMP - 1), g = tid >> 6;        // staging role: pixel of the tile, tap group
  for (int t = T + g; t < TP; t += G) Vs[p * LDV + t] = 0.f;
  const int64_t total = (int64_t)y.N * y.H * y.W;
  const int64_t ntiles = (total + BMP - 1) / BMP;
  float v[NV];
  auto issue = [&](int64_t tile) __attribute__((always_inline)) {
    const int64_t pix = tile * BMP + p;
    const int64_t pc = pix < total ? pix : total - 1;
    const int wo = (int)(pc % y.W);
    const int64_t r = pc / y.W;
    const int ho = (int)(r % y.H), n = (int)(r / y.H);
    const float* base = img + (int64_t)n * 3 * Hi * Wi;
    const int iw0 = wo * stride - pad;
#pragma unroll
    for (int jr = 0; jr < NR; ++jr) {
      const int row = min(g + G * jr, 20), c = row / 7, kh = row - 7 * c;
      const int ih = ho * stride - pad + kh, ihc = min(max(ih, 0), Hi - 1);
      const float* rb = base + ((int64_t)c * Hi + ihc) * Wi;
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) {
        const int iw = iw0 + kw, iwc = min(max(iw, 0), Wi - 1);
        const float q = rb[iwc];
        v[jr * 7 + kw] = (ih == ihc && iw == iwc) ? q : 0.f;
      }
    }
  };
  float s = 0.f, q = 0.f, kk = 0.f;                   // this lane's feature: shifted sums (see TileStat)
  int cnt = 0;
  int64_t tile = blockIdx.x;
  if (tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int jr = 0; jr < NR; ++jr)
      if (g + G * jr < 21)
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) Vs[p * LDV + (g + G * jr) * 7 + kw] = v[jr * 7 + kw];
    __syncthreads();
    if (tile + gridDim.x < ntiles) issue(tile + gridDim.x);
    const f4* ap = reinterpret_cast<const f4*>(Vs + (pg * 32 + l31) * LDV + NKS * lh);
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NKS / 4; ++c) {
      if ((c & 3) == 0) asm volatile("" ::: "memory");      // at most 4 A fragments (16 registers) in flight: hoisted, all 20 spill
      const f4 a = ap[c];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wreg[4 * c + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wreg[4 * c + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wreg[4 * c + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wreg[4 * c + 3], acc, 0, 0, 0);
    }
    const int64_t pbase = tile * BMP + pg * 32 + 4 * lh;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t pix = pbase + (r & 3) + 8 * (r >> 2);
      if (pix < total) {
        y.data[pix * y.cstride + y.coff + co] = acc[r];
        if (cnt == 0) kk = acc[r];
        const float d = acc[r] - kk;
        s += d;
        q += d * d;
        ++cnt;
      }
    }
  }
  if (stats) {
    const double k0 = kk, c0 = cnt;
    double sd = (double)s + c0 * k0, qd = (double)q + 2.0 * k0 * (double)s + c0 * k0 * k0;
    sd += __shfl_xor(sd, 32, 64);
    qd += __shfl_xor(qd, 32, 64);
    __syncthreads();
    if (lh == 0) {
      redd[pg * 2 * CO + co] = sd;
      redd[pg * 2 * CO + CO + co] = qd;
    }
    __syncthreads();
    if (tid < 2 * CO) {
      double* st = stats + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * CO;
      atomicAdd(st + tid, redd[tid] + redd[2 * CO + tid]);
    }
    if (fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block(fin, stats);
  }
}

extern "C" int lhn_conv_stem_fwd(const float* img, const float* w, const lhn_view* y, double* stats, int Hi, int Wi, int k,
                                 int stride, int pad, const lhn_bnfin* finp, void* stream) {
  lhn_bnfin fin;
  if (finp && stats) fin = *finp; else fin.counter = nullptr;
  LHN_CHECK_ARG(img && w && lhn_view_ok(y), "lhn_conv_stem_fwd: bad view / null pointer");
  // (40 = 160 / 4 is admitted by name: the direct kernel's pixel lanes then do not fill the block, see k_stem_fwd)
  LHN_CHECK_ARG(((y->C % 8 == 0 && pow2(y->C / 8)) || y->C == 40) && y->C <= 256, "lhn_conv_stem_fwd: Cout=%d", y->C);
  LHN_CHECK_ARG((k == 1 || k == 3 || k == 5 || k == 7) && stride >= 1, "lhn_conv_stem_fwd: k=%d", k);
  const int Ho = (Hi + 2 * pad - k) / stride + 1, Wo = (Wi + 2 * pad - k) / stride + 1;
  LHN_CHECK_ARG(y->H == Ho && y->W == Wo, "lhn_conv_stem_fwd: output %dx%d, expected %dx%d", y->H, y->W, Ho, Wo);
  const int PL = 256 / (y->C / 8);
  const size_t lds = (size_t)(3 * k * k * y->C) * 4 + 256 * 16 * 4;
  const bool mfma = !lhn_dw_force_gather() && ((k == 7 && y->C == 64) || (k == 3 && y->C == 32));
  // the direct kernel is launched without a dynamic-LDS opt-in: 64 KiB is what a launch may ask for unprepared
  LHN_CHECK_ARG(mfma || lds <= 65536, "lhn_conv_stem_fwd: k=%d Cout=%d needs %zu B of LDS (limit 65536 B)", k, y->C, lds);
  if (k == 7 && y->C == 64 && !lhn_dw_force_gather()) {
    const size_t lds7 = (size_t)64 * 164 * 4 + 2 * 2 * 64 * 8;
    static LhnKernelCfg cfg7;
    int per_cu = 1;
    if (!lhn_kernel_cfg(cfg7, &k_stem7_fwd_mfma, lds7, 3, &per_cu)) {
      lhn_set_error("lhn_conv_stem_fwd: cannot reserve %zu B of LDS", lds7);
      return 2;
    }
    const int64_t ntiles = ((int64_t)y->N * Ho * Wo + 63) / 64;
    int grid = lhn_num_cus() * per_cu;
    if (grid > ntiles) grid = (int)ntiles;
    hipLaunchKernelGGL(k_stem7_fwd_mfma, dim3(grid), dim3(256), lds7, (hipStream_t)stream, img, w, *y, stats, Hi, Wi, stride, pad, fin);
  } else if (k == 3 && y->C == 32 && !lhn_dw_force_gather()) {
    // (3 / 6 / 12 blocks per CU measured in round 3: no difference, forward 2.680 / 2.677 / 2.682 ms)
    hipLaunchKernelGGL(k_stem3_fwd_mfma, dim3(grid_for((int64_t)y->N * Ho * Wo, 256, 3)), dim3(256), 0, (hipStream_t)stream, img, w, *y,
                       stats, Hi, Wi, stride, pad, fin);
  } else
    hipLaunchKernelGGL(k_stem_fwd, dim3(grid_for((int64_t)y->N * Ho * Wo, PL, 8)), dim3(256), lds, (hipStream_t)stream, img,
                       w, *y, stats, Hi, Wi, k, stride, pad, fin);
  LHN_CHECK_LAUNCH("lhn_conv_stem_fwd");
  return 0;
}

// ------------------------------------------------------------------ stem backward (weight gradient; the image gets none)
// dy is formed on the fly:  du = lrelu'(u) * (gate*dz + pooled-gradient),  dy = A*du + B*y + C.
__device__ __forceinline__ f4 dw_load_dy(const lhn_view& y, const lhn_gradview& g, const Xf4& xf, const Gr4& gr,
                                         int64_t pix, int n, int h, int w, int ca) {
  const f4 raw = *reinterpret_cast<const f4*>(y.data + pix * y.cstride + ca);
  const f4 dz = *reinterpret_cast<const f4*>(g.dz + pix * y.cstride + ca);
  const f4 du = lhn_grad_du(y, g, xf, raw, dz, n, h, w, ca);
  return gr.A * du + gr.B * raw + gr.Cc;
}

// stem wgrad: thread = (pixel lane, 4 output channels); T = 3*KR*K accumulators of float4 for the kernel rows
// [kh0, kh0 + KR) (K = 7, hourglassnet.py:100, runs one kernel row per launch: 147 float4 accumulators do not fit)
template <int K, int KR>
__global__ void __launch_bounds__(256) k_stem_bwd(const float* __restrict__ img, lhn_view y, lhn_gradview gy,
                                                  float* __restrict__ dw, int Hi, int Wi, int stride, int pad, int nrep,
                                                  int64_t rep_stride, int kh0) {
  dw += (size_t)(blockIdx.x % nrep) * rep_stride;
  constexpr int T = 3 * KR * K;
  __shared__ f4 red[256];
  const int C4 = y.C >> 2;
  const int tid = threadIdx.x, c4 = tid % C4, pl = tid / C4, PL = 256 / C4;
  const int cy = y.coff + 4 * c4;
  const Xf4 yxf = lhn_load_xf(y, cy);
  const Gr4 ygr = lhn_load_coef(gy, y.cstride, cy);
  f4 acc[T];
#pragma unroll
  for (int i = 0; i < T; ++i) acc[i] = (f4){0.f, 0.f, 0.f, 0.f};
  const int64_t total = (int64_t)y.N * y.H * y.W;
  // (Cout = 40: ten channel groups, 25 pixel lanes, threads 250..255 take no pixel and add zeros)
  for (int64_t pix = pl < PL ? (int64_t)blockIdx.x * PL + pl : total; pix < total; pix += (int64_t)gridDim.x * PL) {
    const int wo = (int)(pix % y.W);
    const int64_t t = pix / y.W;
    const int ho = (int)(t % y.H), n = (int)(t / y.H);
    const f4 dy = dw_load_dy(y, gy, yxf, ygr, pix, n, ho, wo, cy);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* plane = img + ((int64_t)n * 3 + c) * Hi * Wi;
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        const int ih = ho * stride - pad + kh0 + r;
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int iw = wo * stride - pad + kw;
          float v = 0.f;
          if (ih >= 0 && ih < Hi && iw >= 0 && iw < Wi) v = plane[(int64_t)ih * Wi + iw];
          acc[(c * KR + r) * K + kw] += dy * v;
        }
      }
    }
  }
  constexpr int TW = 3 * K * K;            // weights per output channel
#pragma unroll
  for (int i = 0; i < T; ++i) {
    __syncthreads();
    red[tid] = acc[i];
    __syncthreads();
    if (tid < C4) {
      f4 s = (f4){0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < PL; ++j) s += red[j * C4 + tid];
      const int c = i / (KR * K), r = (i / K) % KR, kw = i % K, e = c * K * K + (kh0 + r) * K + kw;
      atomicAdd(dw + (4 * tid + 0) * TW + e, s.x);
      atomicAdd(dw + (4 * tid + 1) * TW + e, s.y);
      atomicAdd(dw + (4 * tid + 2) * TW + e, s.z);
      atomicAdd(dw + (4 * tid + 3) * TW + e, s.w);
    }
  }
}


// ------------------------------------------------------------------ stem weight gradient, 3x3 -> 32 features, on MFMA:
// dW[co][tap] = sum_pixels dy[pixel][co] * patch[pixel][tap] is a (32 x 27) = dY^T (32 x P) * V (P x 27) GEMM with the
// pixels as K.  Per 256-pixel tile the block parks dy (formed on the fly from dz, raw y and the BatchNorm-backward
// coefficients) and the im2col patch (27 taps, padded to 32 zero columns) in LDS; every wave then runs 32
// v_mfma_f32_32x32x2_f32 over its 64 pixels into one 32x32 accumulator that lives across the whole launch.
__global__ void __launch_bounds__(256) k_stem3_bwd_mfma(const float* __restrict__ img, lhn_view y, lhn_gradview gy, float* __restrict__ dw,
                                                        int Hi, int Wi, int stride, int pad, int nrep, int64_t rep_stride) {
  constexpr int CO = 32, LDY = CO + 4, LDV = 33;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dYs = smem;                     // [256][LDY] pixel-major dy; reused for the final cross-wave sum (4096 floats)
  float* Vs = smem + 256 * LDY;          // [256][LDV] pixel-major patch, columns 27..31 stay zero
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int c4 = tid & 7, prow = tid >> 3;
  const int cy = y.coff + 4 * c4;
  const Xf4 yxf = lhn_load_xf(y, cy);
  const Gr4 ygr = lhn_load_coef(gy, y.cstride, cy);
  for (int t = 27; t < 32; ++t) Vs[tid * LDV + t] = 0.f;
  f16v acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int64_t total = (int64_t)y.N * y.H * y.W;
  const int64_t ntiles = (total + 255) / 256;
  // raw loads of a tile go into registers one tile AHEAD (dy is formed when they are parked in LDS)
  f4 yraw[8], zraw[8];
  float v[27];
  auto issue = [&](int64_t tile) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int64_t pix = tile * 256 + prow + 32 * j;
      pix = pix < total ? pix : total - 1;
      yraw[j] = *reinterpret_cast<const f4*>(y.data + pix * y.cstride + cy);
      zraw[j] = *reinterpret_cast<const f4*>(gy.dz + pix * y.cstride + cy);
    }
    const int64_t pix = tile * 256 + tid;
    const int64_t pc = pix < total ? pix : total - 1;
    const int wo = (int)(pc % y.W);
    const int64_t r = pc / y.W;
    const int ho = (int)(r % y.H), n = (int)(r / y.H);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* plane = img + ((int64_t)n * 3 + c) * Hi * Wi;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int ih = ho * stride - pad + kh, ihc = min(max(ih, 0), Hi - 1);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int iw = wo * stride - pad + kw, iwc = min(max(iw, 0), Wi - 1);
          const float t = plane[(int64_t)ihc * Wi + iwc];
          v[c * 9 + kh * 3 + kw] = (ih == ihc && iw == iwc) ? t : 0.f;      // (rows past the end meet dy = 0)
        }
      }
    }
  };
  int64_t tile = blockIdx.x;
  if (tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();                       // the previous tile's MFMA reads are done
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int p = prow + 32 * j;
      const int64_t pix = tile * 256 + p;
      f4 d = (f4){0.f, 0.f, 0.f, 0.f};
      if (pix < total) {
        const int wo = (int)(pix % y.W);
        const int64_t r = pix / y.W;
        const f4 du = lhn_grad_du(y, gy, yxf, yraw[j], zraw[j], (int)(r / y.H), (int)(r % y.H), wo, cy);
        d = ygr.A * du + ygr.B * yraw[j] + ygr.Cc;
      }
      *reinterpret_cast<f4*>(dYs + p * LDY + 4 * c4) = d;
    }
#pragma unroll
    for (int t = 0; t < 27; ++t) Vs[tid * LDV + t] = v[t];
    __syncthreads();
    if (tile + gridDim.x < ntiles) issue(tile + gridDim.x);
    const float* ar = dYs + (wave * 64 + lh) * LDY + l31;
    const float* br = Vs + (wave * 64 + lh) * LDV + l31;
#pragma unroll 8
    for (int ks = 0; ks < 32; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[2 * ks * LDY], br[2 * ks * LDV], acc, 0, 0, 0);
  }
  // cross-wave sum through LDS, then one float atomic per weight into this block's gradient replica
  __syncthreads();
  float* part = dYs;                                 // [4][16][64]
#pragma unroll
  for (int r = 0; r < 16; ++r) part[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
  dw += (size_t)(blockIdx.x % nrep) * rep_stride;
  for (int i = tid; i < CO * 27; i += 256) {
    const int co = i / 27, t = i - co * 27;
    const int r = (co & 3) + 4 * (co >> 3), ln = t + 32 * ((co >> 2) & 1);      // accumulator row co = (r & 3) + 8 (r >> 2) + 4 lh
    const float v = part[(0 * 16 + r) * 64 + ln] + part[(1 * 16 + r) * 64 + ln] + part[(2 * 16 + r) * 64 + ln] + part[(3 * 16 + r) * 64 + ln];
    atomicAdd(dw + i, v);
  }
}


// ------------------------------------------------------------------ stem weight gradient, 7x7 -> 64 features, on MFMA:
// dW (64 x 147) = dY^T (64 x P) * patch (P x 147): 2 feature tiles x 5 tap tiles of 32 x 32 over the four waves (3, 3, 2, 2),
// K = the 64 pixels of a tile.  Staging as in k_stem7_fwd_mfma (row-wise taps) + k_stem3_bwd_mfma (dy formed at commit).
__global__ void __launch_bounds__(256, 2) k_stem7_bwd_mfma(const float* __restrict__ img, lhn_view y, lhn_gradview gy, float* __restrict__ dw,
                                                           int Hi, int Wi, int stride, int pad, int nrep, int64_t rep_stride) {
  constexpr int CO = 64, T = 147, LDY = CO + 4, LDV = 161, BMP = 64, G = 4, NR = 6;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dYs = smem;                     // [BMP][LDY]
  float* Vs = smem + BMP * LDY;          // [BMP][LDV], columns 147..159 stay zero
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int c4 = tid & 15, prow = tid >> 4;
  const int cy = y.coff + 4 * c4;
  const Xf4 yxf = lhn_load_xf(y, cy);
  const Gr4 ygr = lhn_load_coef(gy, y.cstride, cy);
  const int p = tid & (BMP - 1), g = tid >> 6;
  for (int t = T + g; t < 160; t += G) Vs[p * LDV + t] = 0.f;
  f16v acc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const int64_t total = (int64_t)y.N * y.H * y.W;
  const int64_t ntiles = (total + BMP - 1) / BMP;
  f4 yraw[4], zraw[4];
  float v[NR * 7];
  auto issue = [&](int64_t tile) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int64_t pix = tile * BMP + prow + 16 * j;
      pix = pix < total ? pix : total - 1;
      yraw[j] = *reinterpret_cast<const f4*>(y.data + pix * y.cstride + cy);
      zraw[j] = *reinterpret_cast<const f4*>(gy.dz + pix * y.cstride + cy);
    }
    const int64_t pix = tile * BMP + p;
    const int64_t pc = pix < total ? pix : total - 1;
    const int wo = (int)(pc % y.W);
    const int64_t r = pc / y.W;
    const int ho = (int)(r % y.H), n = (int)(r / y.H);
    const float* base = img + (int64_t)n * 3 * Hi * Wi;
    const int iw0 = wo * stride - pad;
#pragma unroll
    for (int jr = 0; jr < NR; ++jr) {
      const int row = min(g + G * jr, 20), c = row / 7, kh = row - 7 * c;
      const int ih = ho * stride - pad + kh, ihc = min(max(ih, 0), Hi - 1);
      const float* rb = base + ((int64_t)c * Hi + ihc) * Wi;
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) {
        const int iw = iw0 + kw, iwc = min(max(iw, 0), Wi - 1);
        const float q = rb[iwc];
        v[jr * 7 + kw] = (ih == ihc && iw == iwc) ? q : 0.f;
      }
    }
  };
  int64_t tile = blockIdx.x;
  if (tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pp = prow + 16 * j;
      const int64_t pix = tile * BMP + pp;
      f4 d = (f4){0.f, 0.f, 0.f, 0.f};
      if (pix < total) {
        const int wo = (int)(pix % y.W);
        const int64_t r = pix / y.W;
        const f4 du = lhn_grad_du(y, gy, yxf, yraw[j], zraw[j], (int)(r / y.H), (int)(r % y.H), wo, cy);
        d = ygr.A * du + ygr.B * yraw[j] + ygr.Cc;
      }
      *reinterpret_cast<f4*>(dYs + pp * LDY + 4 * c4) = d;
    }
#pragma unroll
    for (int jr = 0; jr < NR; ++jr)
      if (g + G * jr < 21)
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) Vs[p * LDV + (g + G * jr) * 7 + kw] = v[jr * 7 + kw];
    __syncthreads();
    if (tile + gridDim.x < ntiles) issue(tile + gridDim.x);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int job = wave + 4 * i;                  // 10 jobs: feature tile = job & 1, tap tile = job >> 1
      if (job < 10) {
        const float* ar = dYs + lh * LDY + (job & 1) * 32 + l31;
        const float* br = Vs + lh * LDV + (job >> 1) * 32 + l31;
#pragma unroll 8
        for (int ks = 0; ks < 32; ++ks) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[2 * ks * LDY], br[2 * ks * LDV], acc[i], 0, 0, 0);
      }
    }
  }
  dw += (size_t)(blockIdx.x % nrep) * rep_stride;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int job = wave + 4 * i;
    if (job < 10) {
      const int t = (job >> 1) * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = (job & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (t < T) atomicAdd(dw + co * T + t, acc[i][r]);
      }
    }
  }
}

extern "C" int lhn_conv_stem_bwd(const float* img, const lhn_view* y, const lhn_gradview* gy, float* dw, int Hi, int Wi, int k,
                                 int stride, int pad, int nrep, int64_t rep_stride, void* stream) {
  if (nrep < 1) nrep = 1;
  LHN_CHECK_ARG(img && lhn_view_ok(y) && gy && gy->dz && dw, "lhn_conv_stem_bwd: bad view / null pointer");
  LHN_CHECK_ARG((pow2(y->C / 4) || y->C == 40) && y->C <= 256 && (k == 1 || k == 3 || k == 7), "lhn_conv_stem_bwd: Cout=%d k=%d", y->C, k);
  const int PL = 256 / (y->C / 4);
  const int g = grid_for((int64_t)y->N * y->H * y->W, PL, 4);
  if (k == 7 && y->C == 64 && !lhn_dw_force_gather()) {
    const size_t lds = (size_t)64 * (68 + 161) * 4;
    static LhnKernelCfg cfg7;
    int per_cu = 1;
    if (!lhn_kernel_cfg(cfg7, &k_stem7_bwd_mfma, lds, 2, &per_cu)) {
      lhn_set_error("lhn_conv_stem_bwd: cannot reserve %zu B of LDS", lds);
      return 2;
    }
    const int64_t ntiles = ((int64_t)y->N * y->H * y->W + 63) / 64;
    int grid = lhn_num_cus() * per_cu;
    if (grid > ntiles) grid = (int)ntiles;
    hipLaunchKernelGGL(k_stem7_bwd_mfma, dim3(grid), dim3(256), lds, (hipStream_t)stream, img, *y, *gy, dw, Hi, Wi, stride, pad, nrep, rep_stride);
  } else if (k == 3 && y->C == 32 && !lhn_dw_force_gather()) {
    const size_t lds = (size_t)256 * (36 + 33) * 4;
    static LhnKernelCfg cfg;
    int per_cu = 1;
    if (!lhn_kernel_cfg(cfg, &k_stem3_bwd_mfma, lds, 2, &per_cu)) {
      lhn_set_error("lhn_conv_stem_bwd: cannot reserve %zu B of LDS", lds);
      return 2;
    }
    const int64_t ntiles = ((int64_t)y->N * y->H * y->W + 255) / 256;
    int grid = lhn_num_cus() * per_cu;
    if (grid > ntiles) grid = (int)ntiles;
    hipLaunchKernelGGL(k_stem3_bwd_mfma, dim3(grid), dim3(256), lds, (hipStream_t)stream, img, *y, *gy, dw, Hi, Wi, stride, pad, nrep, rep_stride);
  } else if (k == 3)
    hipLaunchKernelGGL((k_stem_bwd<3, 3>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, *y, *gy, dw, Hi, Wi, stride, pad, nrep, rep_stride, 0);
  else if (k == 1)
    hipLaunchKernelGGL((k_stem_bwd<1, 1>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, *y, *gy, dw, Hi, Wi, stride, pad, nrep, rep_stride, 0);
  else
    for (int kh = 0; kh < 7; ++kh)
      hipLaunchKernelGGL((k_stem_bwd<7, 1>), dim3(g), dim3(256), 0, (hipStream_t)stream, img, *y, *gy, dw, Hi, Wi, stride, pad, nrep, rep_stride, kh);
  LHN_CHECK_LAUNCH("lhn_conv_stem_bwd");
  return 0;
}
