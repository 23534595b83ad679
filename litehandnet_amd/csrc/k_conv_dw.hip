// Depthwise k x k convolution (stride, dilation), NHWC fp32.
// HBM-bound: each thread owns 4 channels of one output pixel and gathers its taps through L1/L2
// (neighbouring outputs share them), applying the producer's pending BatchNorm/activation on load;
// the epilogue accumulates this layer's BatchNorm statistics (one double atomic per block+channel).
#include <stdlib.h>
#include "lhn_common.h"

// ------------------------------------------------------------------ depthwise forward
// Block = persistent over output rows (n, ho); thread = (c4, pixel lane).  All index math is 32-bit and the
// row/tap validity is block-uniform; a wave reads 64/C4 neighbouring pixels x C*4 contiguous bytes per tap.
template <int K>
__global__ void __launch_bounds__(256) k_dw_fwd(lhn_view x, const float* __restrict__ w, lhn_view y,
                                                double* __restrict__ stats, int stride, int pad, int dil, lhn_bnfin fin,
                                                int /*unused*/) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int C = x.C, C4 = C >> 2;
  constexpr int KK = K * K;
  float* Ws = smem;                                   // [KK][C]
  f4* red = reinterpret_cast<f4*>(smem + KK * C);     // [256][2]
  const int tid = threadIdx.x;
  const int c4 = tid % C4, pl = tid / C4, PL = 256 / C4;
  const int cin = x.coff + 4 * c4, cout = y.coff + 4 * c4;
  // pending BatchNorm of the input (LDS: >= 8 KB, weights staged after)
  const Xf4 xf = lhn_load_xf(x, cin);
  for (int i = tid; i < KK * C; i += 256) {
    const int c = i / KK, t = i - c * KK;
    Ws[t * C + c] = w ? w[i] : 1.f;
  }
  __syncthreads();
  f4 wt[KK];
#pragma unroll
  for (int t = 0; t < KK; ++t) wt[t] = *reinterpret_cast<const f4*>(Ws + t * C + 4 * c4);
  const int rows = y.N * y.H;
  double sd[4] = {0, 0, 0, 0}, qd[4] = {0, 0, 0, 0};      // per-row fp32 partials promoted to double (see k_conv_pw.hip)
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int n = row / y.H, ho = row - n * y.H;
    const float* xin = x.data + (size_t)n * x.H * x.W * x.cstride + cin;
    f4 gate = (f4){1.f, 1.f, 1.f, 1.f};
    if (x.gate) gate = *reinterpret_cast<const f4*>(x.gate + (size_t)n * x.cstride + cin);
    float* yout = y.data + (size_t)row * y.W * y.cstride + cout;
    f4 s = (f4){0.f, 0.f, 0.f, 0.f}, q = s, kk = s;     // shifted by the row's first value (see TileStat)
    int cnt = 0;
    for (int wo = LHN_LANE0(pl, PL); wo < y.W; wo += PL) {
      f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
      // branch-free taps: clamped (always in-bounds) addresses, so all K*K loads issue back to back
      f4 raw[KK];
      bool ok[KK];
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        const int ih = ho * stride - pad + kh * dil;
        const int ihc = min(max(ih, 0), x.H - 1);
        const float* xr = xin + (size_t)ihc * x.W * x.cstride;
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int iw = wo * stride - pad + kw * dil;
          const int iwc = min(max(iw, 0), x.W - 1);
          ok[kh * K + kw] = (ih == ihc) && (iw == iwc);
          raw[kh * K + kw] = *reinterpret_cast<const f4*>(xr + iwc * x.cstride);
        }
      }
#pragma unroll
      for (int t = 0; t < KK; ++t) {
        const f4 v = lhn_apply_xf(raw[t], xf) * gate;
        acc += (ok[t] ? v : (f4){0.f, 0.f, 0.f, 0.f}) * wt[t];
      }
      *reinterpret_cast<f4*>(yout + wo * y.cstride) = acc;
      if (cnt == 0) kk = acc;
      const f4 d = acc - kk;
      s += d;
      q += d * d;
      ++cnt;
    }
    lhn_unshift4(sd, qd, s, q, kk, cnt);
  }
  if (stats) {
    double* st = stats + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * C;
    double* redd = reinterpret_cast<double*>(red);          // [256][2] float4 = 1024 doubles
    if (C4 <= 32 && (C4 & (C4 - 1)) == 0) {
      lhn_block_stat_atomics_d(sd, qd, C4, redd, st, st + C);
    } else {                                                // any other C: one LDS slot per (channel group, pixel lane)
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        redd[tid * 4 + j] = sd[j];
      }
      __syncthreads();
      double ts[4] = {0, 0, 0, 0};
      if (tid < C4)
        for (int j = 0; j < PL; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) ts[e] += redd[(j * C4 + tid) * 4 + e];
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) redd[tid * 4 + j] = qd[j];
      __syncthreads();
      if (tid < C4) {
        double tq[4] = {0, 0, 0, 0};
        for (int j = 0; j < PL; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) tq[e] += redd[(j * C4 + tid) * 4 + e];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          atomicAdd(st + 4 * tid + j, ts[j]);
          atomicAdd(st + C + 4 * tid + j, tq[j]);
        }
      }
    }
    if (fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block(fin, stats);
  }
}

// One extra input source: the consumed input is coef[0]*value(x) + coef[1]*value(ex.v) (MSRB's `out + ca(cat)`,
// litehourglass.py:41-45, summed while the halo tile is staged instead of being written by an elementwise pass).
struct DwExtra {
  lhn_view v;
  float coef[2];
  int n;             // 0 or 1
  float* sum_out;    // the summed input (tile interiors) is also written here, or NULL (lhn_pw_opts.sum_out)
  int so_cstride, so_coff;
};

// =====================================================================================================
// Backward.  dy is formed on the fly:  du = lrelu'(u) * (gate*dz + pooled-gradient),  dy = A*du + B*y + C.
// row-local dy loader: off = element offset of (n, h, w, channel ca) inside the y buffer
__device__ __forceinline__ f4 dw_dy_at(const lhn_view& y, const lhn_gradview& g, const Xf4& xf, const Gr4& gr, f4 gate,
                                       size_t off, int n, int h, int w, int ca) {
  const f4 raw = *reinterpret_cast<const f4*>(y.data + off);
  f4 e = *reinterpret_cast<const f4*>(g.dz + off) * gate;
  const f4 u = raw * xf.sc + xf.sh;
  const f4 dl = (f4){u.x > 0.f ? 1.f : xf.sl.x, u.y > 0.f ? 1.f : xf.sl.y, u.z > 0.f ? 1.f : xf.sl.z, u.w > 0.f ? 1.f : xf.sl.w};
  if (g.dpool) e += lhn_dpool_sum(g, y, n, h, w, ca);
  const f4 du = e * dl;
  return gr.A * du + gr.B * raw + gr.Cc;
}

// dgrad: block = persistent over INPUT rows (n, hi); thread = (c4, pixel lane)
template <int K>
__global__ void __launch_bounds__(256) k_dw_bwd_data(lhn_view x, const float* __restrict__ w, lhn_view y, lhn_gradview gy,
                                                     float* __restrict__ dx, int accumulate, int stride, int pad, int dil) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int C = x.C, C4 = C >> 2;
  constexpr int KK = K * K;
  float* Ws = smem;
  const int tid = threadIdx.x;
  for (int i = tid; i < KK * C; i += 256) {
    const int c = i / KK, t = i - c * KK;
    Ws[t * C + c] = w ? w[i] : 1.f;
  }
  __syncthreads();
  const int c4 = tid % C4, pl = tid / C4, PL = 256 / C4;
  const int cx = x.coff + 4 * c4, cy = y.coff + 4 * c4;
  const Xf4 yxf = lhn_load_xf(y, cy);
  const Gr4 ygr = lhn_load_coef(gy, y.cstride, cy);
  f4 wt[KK];
#pragma unroll
  for (int t = 0; t < KK; ++t) wt[t] = *reinterpret_cast<const f4*>(Ws + t * C + 4 * c4);
  const int rows = x.N * x.H;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int n = row / x.H, hi = row - n * x.H;
    f4 gate = (f4){1.f, 1.f, 1.f, 1.f};
    if (y.gate) gate = *reinterpret_cast<const f4*>(y.gate + (size_t)n * y.cstride + cy);
    float* dxr = dx + (size_t)row * x.W * x.cstride + cx;
    for (int wi = LHN_LANE0(pl, PL); wi < x.W; wi += PL) {
      f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        const int hn = hi + pad - kh * dil;
        if (hn < 0 || (stride > 1 && hn % stride)) continue;
        const int ho = hn / stride;
        if (ho >= y.H) continue;
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int wn = wi + pad - kw * dil;
          if (wn < 0 || (stride > 1 && wn % stride)) continue;
          const int wo = wn / stride;
          if (wo >= y.W) continue;
          const size_t off = ((size_t)(n * y.H + ho) * y.W + wo) * y.cstride + cy;
          acc += dw_dy_at(y, gy, yxf, ygr, gate, off, n, ho, wo, cy) * wt[kh * K + kw];
        }
      }
      float* o = dxr + wi * x.cstride;
      if (accumulate) acc += *reinterpret_cast<const f4*>(o);
      *reinterpret_cast<f4*>(o) = acc;
    }
  }
}

// wgrad: block = persistent over OUTPUT rows; thread = (c4, pixel lane); KR kernel rows [kh0, kh0+KR) per launch
template <int K, int KR>
__global__ void __launch_bounds__(256) k_dw_bwd_weight(lhn_view x, lhn_view y, lhn_gradview gy, float* __restrict__ dw,
                                                       int stride, int pad, int dil, int kh0, int nrep, int64_t rep_stride) {
  dw += (size_t)(blockIdx.x % nrep) * rep_stride;
  __shared__ f4 red[256];
  const int C4 = x.C >> 2;
  const int tid = threadIdx.x, c4 = tid % C4, pl = tid / C4, PL = 256 / C4;
  const int cx = x.coff + 4 * c4, cy = y.coff + 4 * c4;
  const Xf4 xxf = lhn_load_xf(x, cx), yxf = lhn_load_xf(y, cy);
  const Gr4 ygr = lhn_load_coef(gy, y.cstride, cy);
  f4 acc[KR * K];
#pragma unroll
  for (int i = 0; i < KR * K; ++i) acc[i] = (f4){0.f, 0.f, 0.f, 0.f};
  const int rows = y.N * y.H;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int n = row / y.H, ho = row - n * y.H;
    f4 ygate = (f4){1.f, 1.f, 1.f, 1.f}, xgate = ygate;
    if (y.gate) ygate = *reinterpret_cast<const f4*>(y.gate + (size_t)n * y.cstride + cy);
    if (x.gate) xgate = *reinterpret_cast<const f4*>(x.gate + (size_t)n * x.cstride + cx);
    const float* xin = x.data + (size_t)n * x.H * x.W * x.cstride + cx;
    for (int wo = LHN_LANE0(pl, PL); wo < y.W; wo += PL) {
      const size_t off = ((size_t)row * y.W + wo) * y.cstride + cy;
      f4 raw[KR * K];
      bool ok[KR * K];
#pragma unroll
      for (int r = 0; r < KR; ++r) {
        const int ih = ho * stride - pad + (kh0 + r) * dil;
        const int ihc = min(max(ih, 0), x.H - 1);
        const float* xr = xin + (size_t)ihc * x.W * x.cstride;
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int iw = wo * stride - pad + kw * dil;
          const int iwc = min(max(iw, 0), x.W - 1);
          ok[r * K + kw] = (ih == ihc) && (iw == iwc);
          raw[r * K + kw] = *reinterpret_cast<const f4*>(xr + iwc * x.cstride);
        }
      }
      const f4 dy = dw_dy_at(y, gy, yxf, ygr, ygate, off, n, ho, wo, cy);
#pragma unroll
      for (int t = 0; t < KR * K; ++t) {
        const f4 v = lhn_apply_xf(raw[t], xxf) * xgate;
        acc[t] += dy * (ok[t] ? v : (f4){0.f, 0.f, 0.f, 0.f});
      }
    }
  }
#pragma unroll
  for (int i = 0; i < KR * K; ++i) {
    __syncthreads();
    red[tid] = acc[i];
    __syncthreads();
    if (tid < C4) {
      f4 s = (f4){0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < PL; ++j) s += red[j * C4 + tid];
      const int tap = (kh0 + i / K) * K + (i % K);
      atomicAdd(dw + (4 * tid + 0) * K * K + tap, s.x);
      atomicAdd(dw + (4 * tid + 1) * K * K + tap, s.y);
      atomicAdd(dw + (4 * tid + 2) * K * K + tap, s.z);
      atomicAdd(dw + (4 * tid + 3) * K * K + tap, s.w);
    }
  }
}

// =====================================================================================================
// LDS-staged K x K depthwise (stride 1, dilation DIL, pad DIL*(K-1)/2) over 32-channel groups.
// Block tile = TH x TW output pixels x 32 channels; the (TH+2P) x (TW+2P) input halo tile is loaded ONCE,
// transformed (pending BN / activation / gate) once, and parked in LDS; every thread (= 4 channels x one
// output column) walks down the tile rows (3x3/dil 1: sliding register window, 3 ds_read_b128 per output).
template <int K, int DIL, int TH, int TW>
struct DwTile {
  static constexpr int P = DIL * (K - 1) / 2, HH = TH + 2 * P, WW = TW + 2 * P, PIX = HH * WW;
};

// FIN: x is the output of a convolution + BatchNorm whose statistics are complete and whose table is not written yet (lhn_bnfinsrc):
// the workgroup folds the replicas of its own 32 channels while its first tile's loads are in flight (the statistics' own loads go
// out in front of them), in LDS the first commit has not touched yet
// (16 KB of the halo tile for the pairs, 384 B of `red` for the table entries), and the first workgroup of each channel group also
// stores what lhn_bn_finalize leaves in memory.  A template flag: the instances that do not fold keep their registers.
template <int K, int DIL, int NS = 1, bool FIN = false>
__global__ void __launch_bounds__(256) k_dwk_fwd_lds(lhn_view x, const float* __restrict__ w, lhn_view y,
                                                     double* __restrict__ stats, int tiles_h, int tiles_w, int cgroups,
                                                     lhn_bnfin fin, int ps, DwExtra ex, int xchunk, lhn_bnfinsrc fs) {
  constexpr int TH = 8, TW = 32, KK = K * K;
  // XCD-aware tile order: blocks are dealt round-robin over the 8 XCDs, so logical block (b % 8) * xchunk + b / 8 gives each
  // XCD a CONTIGUOUS run of tiles -- neighbouring tiles (which share their halo rows / columns) then meet in one L2
  const int bid = xchunk ? (int)(blockIdx.x & 7) * xchunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  using T = DwTile<K, DIL, TH, TW>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f4* tile = reinterpret_cast<f4*>(smem);                  // [PIX][8] float4
  f4* red = tile + T::PIX * 8;                             // [256][2]
  f4* wl = red + 512;                                      // [KK][8] weights of this block's channel group
  const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;   // pl = output column 0..31
  // ps = pixel stride of the lattice a tile lives on.  ps == 2 runs a dilation-2 convolution as FOUR independent
  // dilation-1 convolutions on the parity sub-lattices (pixels (2i+a, 2j+b) only meet pixels of the same parity): the halo
  // shrinks from (TH+4)(TW+4) to (TH+2)(TW+2) and every pixel still is one contiguous 128-byte channel group.
  const int ntile = y.N * ps * ps * tiles_h * tiles_w * cgroups;
  const int cg = bid % cgroups;                            // grid % cgroups == 0 (host): fixed per block
  // C % 32 != 0 (lite_hrnet.py: 20 / 40 / 80 channels): the last group has cvalid < 8 float4 lanes; the others load the
  // group's first lane again (valid memory) and neither store nor count
  const int cvalid = min(8, (x.C - cg * 32) >> 2);
  const bool cok = c4 < cvalid;
  const int c4e = cok ? c4 : 0;
  const int cin = x.coff + cg * 32 + 4 * c4e, cout = y.coff + cg * 32 + 4 * c4e;
  const int cin2 = NS > 1 ? ex.v.coff + cg * 32 + 4 * c4e : 0;
  Xf4 xf, xf2;        // filled after the first tile's loads have been issued (pending BatchNorms are finalized meanwhile)
  for (int i = tid; i < KK * 8; i += 256) {
    const int k = i >> 3, cc = cg * 32 + 4 * min(i & 7, cvalid - 1);
    wl[i] = (f4){w[(cc + 0) * KK + k], w[(cc + 1) * KK + k], w[(cc + 2) * KK + k], w[(cc + 3) * KK + k]};
  }
  double sd[4] = {0, 0, 0, 0}, qd[4] = {0, 0, 0, 0};      // per-tile fp32 partials promoted to double (see k_conv_pw.hip)
  // halo staging in two phases: issue() sends every global load of a tile (clamped coordinates, no branches, so they
  // are all in flight together) into registers one tile AHEAD; commit() transforms, zeroes the padding and writes LDS
  constexpr int NIT = (T::PIX + 31) / 32;
  f4 raw[NIT], raw2[NS > 1 ? NIT : 1];
  auto issue = [&](int t) __attribute__((always_inline)) {
    int r = t / cgroups;
    const int tw = r % tiles_w;
    r /= tiles_w;
    const int th = r % tiles_h;
    r /= tiles_h;
    const int par = r % (ps * ps), n = r / (ps * ps), pa = par / ps, pb = par % ps;
    const int SH = (x.H - pa + ps - 1) / ps, SW = (x.W - pb + ps - 1) / ps;     // sub-lattice extent
    const int h0 = th * TH - T::P, w0 = tw * TW - T::P;
    const float* xin = x.data + (size_t)n * x.H * x.W * x.cstride + cin;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = min(pl + 32 * it, T::PIX - 1);
      const int ph = i / T::WW, pw = i - ph * T::WW;
      const int ih = pa + ps * min(max(h0 + ph, 0), max(SH - 1, 0)), iw = pb + ps * min(max(w0 + pw, 0), max(SW - 1, 0));
      const size_t pix = (size_t)min(ih, x.H - 1) * x.W + min(iw, x.W - 1);
      raw[it] = *reinterpret_cast<const f4*>(xin + pix * x.cstride);
    }
  };
  // second source: loaded at commit time, NOT a tile ahead (44 more live registers would drop the kernel to one block per
  // CU); the other resident block covers the latency
  auto issue2 = [&](int t) __attribute__((always_inline)) {
    int r = t / cgroups;
    const int tw = r % tiles_w;
    r /= tiles_w;
    const int th = r % tiles_h;
    r /= tiles_h;
    const int par = r % (ps * ps), n = r / (ps * ps), pa = par / ps, pb = par % ps;
    const int SH = (x.H - pa + ps - 1) / ps, SW = (x.W - pb + ps - 1) / ps;
    const int h0 = th * TH - T::P, w0 = tw * TW - T::P;
    const float* xin2 = ex.v.data + (size_t)n * x.H * x.W * ex.v.cstride + cin2;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = min(pl + 32 * it, T::PIX - 1);
      const int ph = i / T::WW, pw = i - ph * T::WW;
      const int ih = pa + ps * min(max(h0 + ph, 0), max(SH - 1, 0)), iw = pb + ps * min(max(w0 + pw, 0), max(SW - 1, 0));
      raw2[it] = *reinterpret_cast<const f4*>(xin2 + ((size_t)min(ih, x.H - 1) * x.W + min(iw, x.W - 1)) * ex.v.cstride);
    }
  };
  int t = bid;
  double fa[FIN ? 4 : 1], fb[FIN ? 4 : 1];      // FIN: this thread's share of the statistics, loaded in front of the tile (lhn_common.h)
  LhnFinPre pre;
  if constexpr (FIN) {
    pre = lhn_bn_fin_pre(fs, cg * 32, 4 * cvalid, bid < cgroups);
    lhn_bn_fin_load<4>(fs.stats, fs.C, cg * 32, 4 * cvalid, fa, fb);
  }
  if (t < ntile) issue(t);
  // (the tile region is free until the first commit, which follows a barrier)
  if constexpr (FIN) {
    static_assert(NS == 1 && T::PIX * 8 * 16 >= LHN_STAT_REPLICAS * 32 * 16, "the halo tile holds the replica pairs of one channel group");
    double* rawd = reinterpret_cast<double*>(tile);
    float* tab = reinterpret_cast<float*>(red);
    const int nc = 4 * cvalid;
    const bool lead = bid < cgroups;
    lhn_bn_fin_put<4>(fa, fb, nc, rawd);
    __syncthreads();
    if (tid < nc) {
      double s1, s2;
      lhn_bn_fin_sum_any(rawd, nc, tid, fs.C, s1, s2);
      lhn_bn_fin_channel(fs, pre, s1, s2, cg * 32, tid, lead, tab, 32);
    }
    __syncthreads();
    xf = lhn_bn_fin_xf(tab, 32, 4 * c4e);
  } else {
    xf = lhn_load_xf(x, cin);
  }
  if (NS > 1) xf2 = lhn_load_xf(ex.v, cin2);
  for (; t < ntile; t += gridDim.x) {
    int r = t / cgroups;
    const int tw = r % tiles_w;
    r /= tiles_w;
    const int th = r % tiles_h;
    r /= tiles_h;
    const int par = r % (ps * ps), n = r / (ps * ps), pa = par / ps, pb = par % ps;
    const int SH = (x.H - pa + ps - 1) / ps, SW = (x.W - pb + ps - 1) / ps;
    f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (size_t)n * x.cstride + cin) : (f4){1.f, 1.f, 1.f, 1.f};
    f4 gate2 = (f4){0.f, 0.f, 0.f, 0.f};
    if (NS > 1) {
      gate *= ex.coef[0];
      gate2 = (ex.v.gate ? *reinterpret_cast<const f4*>(ex.v.gate + (size_t)n * ex.v.cstride + cin2) : (f4){1.f, 1.f, 1.f, 1.f}) * ex.coef[1];
    }
    const int h0 = th * TH - T::P, w0 = tw * TW - T::P;
    if (NS > 1) issue2(t);
    __syncthreads();   // previous tile fully consumed (and wl visible)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = pl + 32 * it;
      if (i < T::PIX) {
        const int ph = i / T::WW, pw = i - ph * T::WW;
        const int ih = h0 + ph, iw = w0 + pw;
        const bool inb = ih >= 0 && ih < SH && iw >= 0 && iw < SW;
        f4 v = lhn_apply_xf(raw[it], xf) * gate;
        if (NS > 1) {
          v += lhn_apply_xf(raw2[it], xf2) * gate2;
          if (ex.sum_out && cok && inb && ph >= T::P && ph < T::P + TH && pw >= T::P && pw < T::P + TW)
            *reinterpret_cast<f4*>(ex.sum_out + ((size_t)(n * x.H + pa + ps * ih) * x.W + pb + ps * iw) * ex.so_cstride + ex.so_coff +
                                   cg * 32 + 4 * c4) = v;
        }
        tile[i * 8 + c4] = inb ? v : (f4){0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();
    if (t + (int)gridDim.x < ntile) issue(t + gridDim.x);
    const int wo = tw * TW + pl;
    f4 s = (f4){0.f, 0.f, 0.f, 0.f}, q = s, kk = s;      // shifted by the tile's first value (see TileStat)
    int cnt = 0;
    if (wo < SW && cok) {
      const f4* col = tile + (pl + T::P) * 8 + c4;    // centre column of this thread, tile row 0
      float* yout = y.data + ((size_t)(n * y.H + pa + ps * th * TH) * y.W + pb + ps * wo) * y.cstride + cout;
      if (K == 3 && DIL == 1) {
        f4 wt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[k] = wl[k * 8 + c4];
        f4 win[3][3];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) win[a + 1][b] = col[(a * T::WW + (b - 1)) * 8];
#pragma unroll
        for (int rr = 0; rr < TH; ++rr) {
#pragma unroll
          for (int b = 0; b < 3; ++b) {
            win[0][b] = win[1][b];
            win[1][b] = win[2][b];
            win[2][b] = col[((rr + 2) * T::WW + (b - 1)) * 8];
          }
          if (th * TH + rr < SH) {
            f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
              for (int b = 0; b < 3; ++b) acc += win[a][b] * wt[a * 3 + b];
            *reinterpret_cast<f4*>(yout + (size_t)rr * ps * y.W * y.cstride) = acc;
            if (cnt == 0) kk = acc;
            const f4 d = acc - kk;
            s += d;
            q += d * d;
            ++cnt;
          }
        }
      } else {
        for (int rr = 0; rr < TH; ++rr) {
          if (th * TH + rr >= SH) break;
          f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = 0; b < K; ++b)
              acc += col[((rr + a * DIL) * T::WW + (b * DIL - T::P)) * 8] * wl[(a * K + b) * 8 + c4];
          *reinterpret_cast<f4*>(yout + (size_t)rr * ps * y.W * y.cstride) = acc;
          if (cnt == 0) kk = acc;
          const f4 d = acc - kk;
          s += d;
          q += d * d;
          ++cnt;
        }
      }
    }
    lhn_unshift4(sd, qd, s, q, kk, cnt);
  }
  if (stats) {
    const int C = x.C;
    double* st = stats + (size_t)((bid / cgroups) % LHN_STAT_REPLICAS) * 2 * C + cg * 32;
    lhn_block_stat_atomics_d(sd, qd, 8, reinterpret_cast<double*>(red), st, st + C, cvalid);
    if (fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block_par(fin, stats, reinterpret_cast<double*>(red));
  }
}

// Fused backward (dgrad + wgrad), TH x TW = 8 x 16: the dy halo tile (formed once per element from dz, raw y and
// the BN-backward coefficients) and the transformed x halo tile sit in LDS.
//   dx[h,w]   = sum_taps dy[h+P-a*DIL, w+P-b*DIL] * wgt[a][b]
//   dW[a][b] += sum_{h,w in tile} dy[h,w] * x[h-P+a*DIL, w-P+b*DIL]
// K = 3 keeps all 9 dW accumulators in registers; K = 7 keeps the per-tile partials in LDS (dws) instead.
// BNS: the input x is the output of a convolution + BatchNorm whose ONLY reader is this depthwise convolution (RepBasicUnit:
// 1x1 -> 3x3 depthwise, litehourglass.py:58-60).  The kernel then holds everything the producer's BatchNorm backward needs
// -- d(value of x) (the dx it just computed), the raw x, its table -- and accumulates sum(du), sum(du * xhat) per channel
// into the producer's replicated sums: the separate lhn_bn_bwd_reduce pass (re-reads x and dx: 134 MB, 20 us per unit at
// 64x64) disappears.
struct DwBnSum {
  double* sums;          // [LHN_STAT_REPLICAS][2][C] of the producer's BatchNorm backward, or NULL
  const float* save;     // [2][C] mean | invstd of the producer
  int C, coff;           // producer channels; channel of the producer that x's first channel is
  const float* add[2];   // gradient buffers (dx's geometry) whose values join the stored dx: d(sum) of residual adds that
                         // read x, so that no separate elementwise pass copies / accumulates them (NULL: none)
};

// FOLD: the instances of the small-map route (lhn_dwk_bwd_lds) take the BatchNorm-backward finalize of y in their prologue
// (lhn_bnbwdsrc, fs.sums != NULL) as k_dw3_bwd_rows does: same helpers, replica order and double arithmetic, the replicas as loaded
// in the dy tile (16 KB of its 23 KB, first written after the tile loop's opening barrier), A | B | C of the block's channel group in
// 24 float4 of LDS behind the other regions; blocks 0 .. cgroups-1 (bid = cg) also write memory.
template <int K, int DIL, bool BNS = false, bool FOLD = false>
__global__ void __launch_bounds__(256) k_dwk_bwd_lds(lhn_view x, const float* __restrict__ w, lhn_view y, lhn_gradview gy,
                                                     float* __restrict__ dx, int dx_acc, float* __restrict__ dw, int tiles_h,
                                                     int tiles_w, int cgroups, int nrep, int64_t rep_stride, int ps, DwBnSum bs, int xchunk,
                                                     lhn_bnbwdsrc fs) {
  constexpr int TH = 8, TW = 16, KK = K * K;
  const int bid = xchunk ? (int)(blockIdx.x & 7) * xchunk + (int)(blockIdx.x >> 3) : (int)blockIdx.x;     // see k_dwk_fwd_lds
  constexpr bool REGACC = (K == 3);
  using T = DwTile<K, DIL, TH, TW>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f4* tdy = reinterpret_cast<f4*>(smem);        // [PIX][8]
  f4* tx = tdy + T::PIX * 8;                    // [PIX][8]
  f4* red = tx + T::PIX * 8;                    // [256]
  f4* wl = red + 256;                           // [KK][8]
  f4* dws = wl + KK * 8;                        // [KK][8]  (K = 7 only) block-level dW partials
  f4* traw = dws + KK * 8;                      // [TH*TW][8] raw x of the tile interior (BNS only)
  f4* tmi = traw + TH * TW * 8;                 // [2][8] mean | invstd of this block's channel group (BNS only)
  float* cfA = reinterpret_cast<float*>(BNS ? tmi + 16 : traw);      // [3][32] A | B | C of this block's channel group (FOLD only)
  const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;
  const int colw = pl & 15, rpar = pl >> 4;
  const int ntile = y.N * ps * ps * tiles_h * tiles_w * cgroups;      // ps: see k_dwk_fwd_lds
  const int cg = bid % cgroups;
  const int cvalid = min(8, (x.C - cg * 32) >> 2);          // see k_dwk_fwd_lds
  const bool cok = c4 < cvalid;
  const int c4e = cok ? c4 : 0;
  const int cx = x.coff + cg * 32 + 4 * c4e, cy = y.coff + cg * 32 + 4 * c4e;
  const Xf4 xxf = lhn_load_xf(x, cx), yxf = lhn_load_xf(y, cy);
  Gr4 ygr;
  if (FOLD && fs.sums) {
    static_assert(!FOLD || T::PIX * 8 * sizeof(f4) >= 2 * LHN_FIN_THREADS * sizeof(double), "dy tile holds the replica fold's partials");
    double* raw = reinterpret_cast<double*>(tdy);
    const int nc = 4 * cvalid;
    const LhnBwdPre pre = lhn_bn_bwd_pre(fs, cg * 32, nc);
    lhn_bn_bwd_fold_raw(fs.sums, fs.stat_channels, cg * 32, nc, raw);
    __syncthreads();
    if (tid < nc)
      lhn_bn_bwd_coef_put(lhn_bn_bwd_coef_raw(raw, nc, lhn_fin_groups(y.C), tid, pre, fs.count), fs, const_cast<float*>(gy.coef), y.cstride,
                          y.coff, cg * 32 + tid, cfA, 32, tid, bid < cgroups);
    __syncthreads();      // (publishes cfA; the tile loop's opening barrier frees the fold's scratch)
    ygr.A = *reinterpret_cast<const f4*>(cfA + 4 * c4e);
    ygr.B = *reinterpret_cast<const f4*>(cfA + 32 + 4 * c4e);
    ygr.Cc = *reinterpret_cast<const f4*>(cfA + 64 + 4 * c4e);
  } else {
    ygr = lhn_load_coef(gy, y.cstride, cy);
  }
  for (int i = tid; i < KK * 8; i += 256) {
    const int k = i >> 3, cc = cg * 32 + 4 * min(i & 7, cvalid - 1);
    wl[i] = (f4){w[(cc + 0) * KK + k], w[(cc + 1) * KK + k], w[(cc + 2) * KK + k], w[(cc + 3) * KK + k]};
    if (!REGACC) dws[i] = (f4){0.f, 0.f, 0.f, 0.f};
  }
  f4 accw[REGACC ? KK : 1];
#pragma unroll
  for (int k = 0; k < (REGACC ? KK : 1); ++k) accw[k] = (f4){0.f, 0.f, 0.f, 0.f};
  f4 sdu = (f4){0.f, 0.f, 0.f, 0.f}, sdux = sdu;
  if (BNS && tid < 16) {
    const int kind = tid >> 3, cc = tid & 7;
    tmi[tid] = *reinterpret_cast<const f4*>(bs.save + kind * bs.C + bs.coff + cg * 32 + 4 * cc);
  }
  for (int t = bid; t < ntile; t += gridDim.x) {
    int r = t / cgroups;
    const int tw = r % tiles_w;
    r /= tiles_w;
    const int th = r % tiles_h;
    r /= tiles_h;
    const int par = r % (ps * ps), n = r / (ps * ps), pa = par / ps, pb = par % ps;
    const int SH = (x.H - pa + ps - 1) / ps, SW = (x.W - pb + ps - 1) / ps;
    const f4 xgate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (size_t)n * x.cstride + cx) : (f4){1.f, 1.f, 1.f, 1.f};
    const f4 ygate = y.gate ? *reinterpret_cast<const f4*>(y.gate + (size_t)n * y.cstride + cy) : (f4){1.f, 1.f, 1.f, 1.f};
    const int h0 = th * TH - T::P, w0 = tw * TW - T::P;
    __syncthreads();
    {
      // all global loads of the halo tile first (clamped, branch-free), then the dy / x transforms and the LDS stores
      constexpr int NIT = (T::PIX + 31) / 32;
      f4 rx[NIT], ry[NIT], rz[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int i = min(pl + 32 * it, T::PIX - 1);
        const int ph = i / T::WW, pw = i - ph * T::WW;
        const int ih = min(pa + ps * min(max(h0 + ph, 0), max(SH - 1, 0)), x.H - 1);
        const int iw = min(pb + ps * min(max(w0 + pw, 0), max(SW - 1, 0)), x.W - 1);
        const size_t pix = (size_t)(n * x.H + ih) * x.W + iw;
        rx[it] = *reinterpret_cast<const f4*>(x.data + pix * x.cstride + cx);
        ry[it] = *reinterpret_cast<const f4*>(y.data + pix * y.cstride + cy);
        rz[it] = *reinterpret_cast<const f4*>(gy.dz + pix * y.cstride + cy);
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int i = pl + 32 * it;
        if (i < T::PIX) {
          const int ph = i / T::WW, pw = i - ph * T::WW;
          const int ih = h0 + ph, iw = w0 + pw;
          const bool inb = ih >= 0 && ih < SH && iw >= 0 && iw < SW;     // stride 1, "same" padding: x and y share geometry
          const f4 vx = lhn_apply_xf(rx[it], xxf) * xgate;
          f4 e = rz[it] * ygate;
          const f4 u = ry[it] * yxf.sc + yxf.sh;
          const f4 dl = (f4){u.x > 0.f ? 1.f : yxf.sl.x, u.y > 0.f ? 1.f : yxf.sl.y, u.z > 0.f ? 1.f : yxf.sl.z,
                             u.w > 0.f ? 1.f : yxf.sl.w};
          if (gy.dpool && inb) e += lhn_dpool_sum(gy, y, n, pa + ps * ih, pb + ps * iw, cy);
          const f4 vy = ygr.A * (e * dl) + ygr.B * ry[it] + ygr.Cc;
          const f4 z = (f4){0.f, 0.f, 0.f, 0.f};
          tx[i * 8 + c4] = inb ? vx : z;
          tdy[i * 8 + c4] = inb ? vy : z;
          if (BNS && ph >= T::P && ph < T::P + TH && pw >= T::P && pw < T::P + TW) traw[((ph - T::P) * TW + pw - T::P) * 8 + c4] = rx[it];
        }
      }
    }
    __syncthreads();
    const int wcol = tw * TW + colw;
    if (REGACC) {
#pragma unroll
      for (int j = 0; j < TH / 2; ++j) {
        const int rr = 2 * j + rpar, hh = th * TH + rr;
        if (wcol < SW && hh < SH) {
          const int centre = ((rr + T::P) * T::WW + colw + T::P) * 8 + c4;
          const f4 dyc = tdy[centre];
          f4 accx = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = 0; b < K; ++b) {
              const int off = ((a * DIL - T::P) * T::WW + (b * DIL - T::P)) * 8;
              accx += tdy[centre - off] * wl[(a * K + b) * 8 + c4];
              accw[REGACC ? a * K + b : 0] += dyc * tx[centre + off];
            }
          if (BNS) {          // accx is the complete d(value of x): this kernel is x's only reader (host-checked, dx_acc == 0)
            const f4 raw = traw[(rr * TW + colw) * 8 + c4];
            const f4 u = raw * xxf.sc + xxf.sh;
            const f4 du = accx * (f4){u.x > 0.f ? 1.f : xxf.sl.x, u.y > 0.f ? 1.f : xxf.sl.y, u.z > 0.f ? 1.f : xxf.sl.z, u.w > 0.f ? 1.f : xxf.sl.w};
            sdu += du;
            sdux += du * ((raw - tmi[c4]) * tmi[8 + c4]);
          }
          if (dx && cok) {
            // (issuing these loads for all four rows BEFORE the tap loops -- one memory latency per tile instead of four -- was
            // measured: 2 more spilled registers in the BNS instance and variant B 8.19 -> 8.29 ms per step; not kept)
            float* o = dx + ((size_t)(n * x.H + pa + ps * hh) * x.W + pb + ps * wcol) * x.cstride + cx;
            if (dx_acc) accx += *reinterpret_cast<const f4*>(o);
            if (bs.add[0]) accx += *reinterpret_cast<const f4*>(bs.add[0] + (o - dx));
            if (bs.add[1]) accx += *reinterpret_cast<const f4*>(bs.add[1] + (o - dx));
            *reinterpret_cast<f4*>(o) = accx;
          }
        }
      }
    } else {
      // dgrad
      if (dx)
        for (int j = 0; j < TH / 2; ++j) {
          const int rr = 2 * j + rpar, hh = th * TH + rr;
          if (wcol < SW && hh < SH && cok) {
            const int centre = ((rr + T::P) * T::WW + colw + T::P) * 8 + c4;
            f4 accx = (f4){0.f, 0.f, 0.f, 0.f};
            for (int a = 0; a < K; ++a)
#pragma unroll
              for (int b = 0; b < K; ++b)
                accx += tdy[centre - ((a * DIL - T::P) * T::WW + (b * DIL - T::P)) * 8] * wl[(a * K + b) * 8 + c4];
            float* o = dx + ((size_t)(n * x.H + pa + ps * hh) * x.W + pb + ps * wcol) * x.cstride + cx;
            if (dx_acc) accx += *reinterpret_cast<const f4*>(o);
            if (bs.add[0]) accx += *reinterpret_cast<const f4*>(bs.add[0] + (o - dx));
            if (bs.add[1]) accx += *reinterpret_cast<const f4*>(bs.add[1] + (o - dx));
            *reinterpret_cast<f4*>(o) = accx;
          }
        }
      // wgrad: one kernel row at a time, K register accumulators, cross-lane sum through `red`
      for (int a = 0; a < K; ++a) {
        f4 ar[K];
#pragma unroll
        for (int b = 0; b < K; ++b) ar[b] = (f4){0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < TH / 2; ++j) {
          const int rr = 2 * j + rpar, hh = th * TH + rr;
          if (wcol < SW && hh < SH) {
            const int centre = ((rr + T::P) * T::WW + colw + T::P) * 8 + c4;
            const f4 dyc = tdy[centre];
#pragma unroll
            for (int b = 0; b < K; ++b) ar[b] += dyc * tx[centre + ((a * DIL - T::P) * T::WW + (b * DIL - T::P)) * 8];
          }
        }
#pragma unroll
        for (int b = 0; b < K; ++b) {
          // reduce over the 32 pixel lanes of each channel lane: xor-shuffle across lanes 8,16,32 then LDS for the 4 waves
          f4 v = ar[b];
#pragma unroll
          for (int o = 8; o < 64; o <<= 1) {
            v.x += __shfl_xor(v.x, o, 64);
            v.y += __shfl_xor(v.y, o, 64);
            v.z += __shfl_xor(v.z, o, 64);
            v.w += __shfl_xor(v.w, o, 64);
          }
          if ((tid & 63) < 8) red[(tid >> 6) * 8 + c4 + 32 * b] = v;
        }
        __syncthreads();
        if (tid < 8 * K) {
          const int b = tid >> 3, cc = tid & 7;
          dws[(a * K + b) * 8 + cc] += red[cc + 32 * b] + red[8 + cc + 32 * b] + red[16 + cc + 32 * b] + red[24 + cc + 32 * b];
        }
        __syncthreads();
      }
    }
  }
  if (BNS) {           // BatchNorm-backward sums of the producer: same block reduction as the forward statistics
    double* st = bs.sums + (size_t)((bid / cgroups) % LHN_STAT_REPLICAS) * 2 * bs.C + bs.coff + cg * 32;
    lhn_block_stat_atomics(sdu, sdux, 8, red, st, st + bs.C);
  }
  // ---- flush dW
  float* dwr = dw + (size_t)((bid / cgroups) % nrep) * rep_stride;
  if (REGACC) {
    // lanes of a wave that share c4 (lane bits 3..5 differ) meet by xor-shuffles, the four waves through LDS (the dy tile
    // is dead by now), then one thread per (tap, c4) adds four floats
#pragma unroll
    for (int k = 0; k < KK; ++k)
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) {
        accw[k].x += __shfl_xor(accw[k].x, o, 64);
        accw[k].y += __shfl_xor(accw[k].y, o, 64);
        accw[k].z += __shfl_xor(accw[k].z, o, 64);
        accw[k].w += __shfl_xor(accw[k].w, o, 64);
      }
    __syncthreads();
    if ((tid & 63) < 8)
#pragma unroll
      for (int k = 0; k < KK; ++k) tdy[(k * 4 + (tid >> 6)) * 8 + c4] = accw[k];
    __syncthreads();
    if (tid < KK * 8) {
      const int k = tid >> 3, cc = tid & 7;
      const f4 sacc = tdy[(k * 4 + 0) * 8 + cc] + tdy[(k * 4 + 1) * 8 + cc] + tdy[(k * 4 + 2) * 8 + cc] + tdy[(k * 4 + 3) * 8 + cc];
      const int cb = cg * 32 + 4 * cc;
      if (cc < cvalid) {
        atomicAdd(dwr + (cb + 0) * KK + k, sacc.x);
        atomicAdd(dwr + (cb + 1) * KK + k, sacc.y);
        atomicAdd(dwr + (cb + 2) * KK + k, sacc.z);
        atomicAdd(dwr + (cb + 3) * KK + k, sacc.w);
      }
    }
  } else {
    __syncthreads();
    for (int i = tid; i < KK * 8; i += 256) {
      const int k = i >> 3, cb = cg * 32 + 4 * (i & 7);
      const f4 v = dws[i];
      if ((i & 7) >= cvalid) continue;
      atomicAdd(dwr + (cb + 0) * KK + k, v.x);
      atomicAdd(dwr + (cb + 1) * KK + k, v.y);
      atomicAdd(dwr + (cb + 2) * KK + k, v.z);
      atomicAdd(dwr + (cb + 3) * KK + k, v.w);
    }
  }
}

// Row-streaming fused backward of the 3x3 depthwise convolution (dgrad + wgrad, the fusions of k_dwk_bwd_lds with the same
// meaning).  A work item is a strip of 32 output columns x CH rows x 32 channels of one (image, parity sub-lattice); the
// workgroup walks down it ONE halo row per step.  LDS keeps a ring of R = 2*DIL + 2 rows of dy and of x (the 2*DIL + 1 rows
// the taps read plus the row being written); each step
//   issue the gradient addends of the output row -> commit the halo row loaded one step earlier (dy / x transforms, ring
//   slot q % R) -> issue the next halo row's global loads -> barrier -> taps of the output row -> store dx,
// so a row's loads are in flight while the previous row's taps run, and one barrier per row is the only synchronisation
// (the slot written at step q + 1 is the one the taps of step q - 1 read last).  The last step of an item issues the first
// halo row of the workgroup's next item.  Halo overhead is (32 + 2*DIL) / 32 x (CH + 2*DIL) / CH (1.20 at CH = 16) instead of
// 1.41 for the 8 x 16 tile; per-channel constants and weights are read from LDS, so the kernel fits 4 waves per SIMD.
template <int DIL, bool BNS = false>
__global__ void __launch_bounds__(256, (BNS || DIL > 1) ? 2 : 3) k_dw3_bwd_rows(lhn_view x, const float* __restrict__ w, lhn_view y, lhn_gradview gy,
                                                         float* __restrict__ dx, int dx_acc, float* __restrict__ dw, int nstrips,
                                                         int nchunks, int CH, int cgroups, int nrep, int64_t rep_stride, int ps,
                                                         DwBnSum bs, lhn_bnbwdsrc fs) {
  constexpr int P = DIL, R = 2 * P + 2, WW = 32 + 2 * P, KK = 9;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f4* tdy = reinterpret_cast<f4*>(smem);        // [R][WW][8] dy ring
  f4* tx = tdy + R * WW * 8;                    // [R][WW][8] x ring (consumed value)
  f4* wl = tx + R * WW * 8;                     // [9][8] weights of this block's channel group
  f4* cst = wl + KK * 8;                        // [9][8] x scale | shift | slope, y scale | shift | slope, A | B | C
  f4* tmi = cst + KK * 8;                       // [2][8] mean | invstd of the producer (BNS only)
  f4* traw = tmi + 16;                          // [R][32][8] raw x of the strip's columns (BNS only)
  const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;
  const int ntile = y.N * ps * ps * nchunks * nstrips * cgroups;
  const int cg = blockIdx.x % cgroups;                      // grid % cgroups == 0 (host): fixed per block
  const int cvalid = min(8, (x.C - cg * 32) >> 2);          // see k_dwk_fwd_lds
  const bool cok = c4 < cvalid;
  const int c4e = cok ? c4 : 0;
  const int cx = x.coff + cg * 32 + 4 * c4e, cy = y.coff + cg * 32 + 4 * c4e;
  // every thread loads halo column pl + P of a row (its own output column); threads 0 .. 16*P-1 also load one of the 2*P
  // edge columns 0 .. P-1, 32+P .. 32+2P-1
  const bool edge = tid < 16 * P;
  const int ecol = (pl < P) ? pl : 32 + pl;
  const f4 z = (f4){0.f, 0.f, 0.f, 0.f}, one = (f4){1.f, 1.f, 1.f, 1.f};
  if (tid < KK * 8) {
    const int k = tid >> 3, cc = cg * 32 + 4 * min(tid & 7, cvalid - 1);
    wl[tid] = (f4){w[(cc + 0) * KK + k], w[(cc + 1) * KK + k], w[(cc + 2) * KK + k], w[(cc + 3) * KK + k]};
  } else if (tid < 2 * KK * 8) {
    const int i = tid - KK * 8, kind = i >> 3, ca = cg * 32 + 4 * min(i & 7, cvalid - 1), j = kind % 3;
    const float* tab = kind < 3 ? x.table : kind < 6 ? y.table : gy.coef;
    const int cs = kind < 3 ? x.cstride : y.cstride, co = kind < 3 ? x.coff : y.coff;
    if (kind < 6 || !fs.sums) cst[i] = tab ? *reinterpret_cast<const f4*>(tab + j * cs + co + ca) : ((kind < 6 ? j != 1 : j == 0) ? one : z);
  } else if (BNS && tid < 2 * KK * 8 + 16) {
    const int i = tid - 2 * KK * 8, kind = i >> 3, cc = i & 7;
    tmi[i] = *reinterpret_cast<const f4*>(bs.save + kind * bs.C + bs.coff + cg * 32 + 4 * cc);
  }
  f4 accw[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) accw[k] = z;
  f4 sdu = z, sdux = z;
  // item t -> channel group (fastest: fixed per block), strip, row chunk, parity sub-lattice, image
  struct Item {
    int n, pa, pb, SH, SW, wb, h0, nrows;
  };
  auto decode = [&](int t) __attribute__((always_inline)) {
    Item it;
    int r = t / cgroups;
    const int st = r % nstrips;
    r /= nstrips;
    const int ch = r % nchunks;
    r /= nchunks;
    const int par = r % (ps * ps);
    it.n = r / (ps * ps);
    it.pa = par / ps;
    it.pb = par % ps;
    it.SH = (x.H - it.pa + ps - 1) / ps;
    it.SW = (x.W - it.pb + ps - 1) / ps;
    it.wb = st * 32;
    it.h0 = ch * CH;
    it.nrows = max(0, min(CH, it.SH - it.h0));
    return it;
  };
  // one halo row into registers: raw x, raw y, dz, pooled gradient (main column; edge column), zero outside the map
  f4 mx = z, my = z, mz = z, mp = z, ex = z, ey = z, ez = z, ep = z;
  bool okm = false, oke = false;
  auto issue = [&](const Item& it, int hr) __attribute__((always_inline)) {
    const bool rok = hr >= 0 && hr < it.SH && cok;
    const int ih = it.pa + ps * hr;
    const int cm = it.wb + pl, ce = it.wb - P + ecol;
    okm = rok && cm < it.SW;
    oke = rok && edge && ce >= 0 && ce < it.SW;
    mx = my = mz = mp = ex = ey = ez = ep = z;
    if (okm) {
      const size_t pix = (size_t)(it.n * x.H + ih) * x.W + it.pb + ps * cm;
      mx = *reinterpret_cast<const f4*>(x.data + pix * x.cstride + cx);
      my = *reinterpret_cast<const f4*>(y.data + pix * y.cstride + cy);
      mz = *reinterpret_cast<const f4*>(gy.dz + pix * y.cstride + cy);
      if (gy.dpool) mp = lhn_dpool_sum(gy, y, it.n, ih, it.pb + ps * cm, cy);
    }
    if (oke) {
      const size_t pix = (size_t)(it.n * x.H + ih) * x.W + it.pb + ps * ce;
      ex = *reinterpret_cast<const f4*>(x.data + pix * x.cstride + cx);
      ey = *reinterpret_cast<const f4*>(y.data + pix * y.cstride + cy);
      ez = *reinterpret_cast<const f4*>(gy.dz + pix * y.cstride + cy);
      if (gy.dpool) ep = lhn_dpool_sum(gy, y, it.n, ih, it.pb + ps * ce, cy);
    }
  };
  // transformed values (as k_dwk_bwd_lds) into ring slot s
  auto put = [&](int s, int col, bool ok, f4 rx, f4 ry, f4 rz, f4 rp, f4 xg, f4 yg) __attribute__((always_inline)) {
    const f4 xsc = cst[c4], xsh = cst[8 + c4], xsl = cst[16 + c4];
    const f4 ysc = cst[24 + c4], ysh = cst[32 + c4], ysl = cst[40 + c4];
    const f4 gA = cst[48 + c4], gB = cst[56 + c4], gC = cst[64 + c4];
    const f4 ux = rx * xsc + xsh;
    const f4 vx = (f4){lhn_lrelu(ux.x, xsl.x), lhn_lrelu(ux.y, xsl.y), lhn_lrelu(ux.z, xsl.z), lhn_lrelu(ux.w, xsl.w)} * xg;
    const f4 e = rz * yg + rp;
    const f4 u = ry * ysc + ysh;
    const f4 dl = (f4){u.x > 0.f ? 1.f : ysl.x, u.y > 0.f ? 1.f : ysl.y, u.z > 0.f ? 1.f : ysl.z, u.w > 0.f ? 1.f : ysl.w};
    const f4 vy = gA * (e * dl) + gB * ry + gC;
    tx[(s * WW + col) * 8 + c4] = ok ? vx : z;
    tdy[(s * WW + col) * 8 + c4] = ok ? vy : z;
    if (BNS && col >= P && col < 32 + P) traw[(s * 32 + col - P) * 8 + c4] = rx;
  };
  int t = blockIdx.x;
  if (t < ntile) {
    const Item nx = decode(t);
    issue(nx, nx.h0 - P);
  }
  // BatchNorm-backward finalize of y in the prologue (lhn_bnbwdsrc): A | B | C of this block's channel group straight into cst,
  // the sums' loads behind the first halo row's, the replicas as loaded in the dy ring (16 KB of it, first written after the item
  // loop's opening barrier, which also publishes cst).  Blocks 0 .. cgroups-1 (cg = blockIdx.x) also write memory.
  if (fs.sums) {
    float* cfA = reinterpret_cast<float*>(cst + 6 * 8);
    if (tid >= 4 * cvalid && tid < 32) cfA[tid] = cfA[32 + tid] = cfA[64 + tid] = 0.f;
    double* raw = reinterpret_cast<double*>(tdy);
    const int nc = 4 * cvalid;
    const LhnBwdPre pre = lhn_bn_bwd_pre(fs, cg * 32, nc);
    lhn_bn_bwd_fold_raw(fs.sums, fs.stat_channels, cg * 32, nc, raw);
    __syncthreads();
    if (tid < nc)
      lhn_bn_bwd_coef_put(lhn_bn_bwd_coef_raw(raw, nc, lhn_fin_groups(y.C), tid, pre, fs.count), fs, const_cast<float*>(gy.coef), y.cstride,
                          y.coff, cg * 32 + tid, cfA, 32, tid, (int)blockIdx.x < cgroups);
  }
#pragma unroll 1
  for (; t < ntile; t += gridDim.x) {
    const Item it = decode(t);
    const f4 xg = x.gate ? *reinterpret_cast<const f4*>(x.gate + (size_t)it.n * x.cstride + cx) : one;
    const f4 yg = y.gate ? *reinterpret_cast<const f4*>(y.gate + (size_t)it.n * y.cstride + cy) : one;
    const int wcol = it.wb + pl, nload = it.nrows + 2 * P;
    const bool ocol = wcol < it.SW;
    __syncthreads();     // the previous item's taps are done with the ring (and the constants are visible)
#pragma unroll 1
    for (int q = 0; q < nload; ++q) {
      const bool orow = q >= 2 * P;
      const int hh = it.h0 + max(q - 2 * P, 0);          // output row of this step (q >= 2P)
      float* o = dx + ((size_t)(it.n * x.H + it.pa + ps * hh) * x.W + it.pb + ps * wcol) * x.cstride + cx;
      const bool st = orow && dx && cok && ocol;
      const int s = q % R;
      put(s, pl + P, okm, mx, my, mz, mp, xg, yg);
      if (edge) put(s, ecol, oke, ex, ey, ez, ep, xg, yg);
      if (q + 1 < nload) issue(it, it.h0 - P + q + 1);
      else if (t + (int)gridDim.x < ntile) {
        const Item nx = decode(t + gridDim.x);
        issue(nx, nx.h0 - P);
      }
      __syncthreads();
      if (!orow || !ocol) continue;
      // rows hh - P .. hh + P sit in slots (q - 2P .. q) % R; centre hh in slot (q - P) % R
      int sr[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) sr[a] = (q - 2 * P + a * DIL) % R;
      const int centre = (sr[1] * WW + pl + P) * 8 + c4;
      const f4 dyc = tdy[centre];
      f4 accx = z;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          // dx[h,w] += dy[h+P-a*DIL, w+P-b*DIL] * wgt[a][b] ;  dW[a][b] += dy[h,w] * x[h-P+a*DIL, w-P+b*DIL]
          accx += tdy[(sr[2 - a] * WW + pl + 2 * P - b * DIL) * 8 + c4] * wl[(a * 3 + b) * 8 + c4];
          accw[a * 3 + b] += dyc * tx[(sr[a] * WW + pl + b * DIL) * 8 + c4];
        }
      }
      if (BNS) {          // accx is the complete d(value of x): this kernel is x's only reader (host-checked, dx_acc == 0)
        const f4 raw = traw[(sr[1] * 32 + pl) * 8 + c4];
        const f4 xsc = cst[c4], xsh = cst[8 + c4], xsl = cst[16 + c4];
        const f4 u = raw * xsc + xsh;
        const f4 du = accx * (f4){u.x > 0.f ? 1.f : xsl.x, u.y > 0.f ? 1.f : xsl.y, u.z > 0.f ? 1.f : xsl.z, u.w > 0.f ? 1.f : xsl.w};
        sdu += du;
        sdux += du * ((raw - tmi[c4]) * tmi[8 + c4]);
      }
      if (st) {
        if (dx_acc) accx += *reinterpret_cast<const f4*>(o);
        if (bs.add[0]) accx += *reinterpret_cast<const f4*>(bs.add[0] + (o - dx));
        if (bs.add[1]) accx += *reinterpret_cast<const f4*>(bs.add[1] + (o - dx));
        *reinterpret_cast<f4*>(o) = accx;
      }
    }
  }
  f4* red = tdy;         // the rings are dead after the last item
  if (BNS) {
    double* sts = bs.sums + (size_t)((blockIdx.x / cgroups) % LHN_STAT_REPLICAS) * 2 * bs.C + bs.coff + cg * 32;
    lhn_block_stat_atomics(sdu, sdux, 8, red, sts, sts + bs.C);
  }
  // ---- flush dW (as k_dwk_bwd_lds)
  float* dwr = dw + (size_t)((blockIdx.x / cgroups) % nrep) * rep_stride;
#pragma unroll
  for (int k = 0; k < KK; ++k)
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      accw[k].x += __shfl_xor(accw[k].x, o, 64);
      accw[k].y += __shfl_xor(accw[k].y, o, 64);
      accw[k].z += __shfl_xor(accw[k].z, o, 64);
      accw[k].w += __shfl_xor(accw[k].w, o, 64);
    }
  __syncthreads();
  if ((tid & 63) < 8)
#pragma unroll
    for (int k = 0; k < KK; ++k) red[(k * 4 + (tid >> 6)) * 8 + c4] = accw[k];
  __syncthreads();
  if (tid < KK * 8) {
    const int k = tid >> 3, cc = tid & 7;
    const f4 sacc = red[(k * 4 + 0) * 8 + cc] + red[(k * 4 + 1) * 8 + cc] + red[(k * 4 + 2) * 8 + cc] + red[(k * 4 + 3) * 8 + cc];
    const int cb = cg * 32 + 4 * cc;
    if (cc < cvalid) {
      atomicAdd(dwr + (cb + 0) * KK + k, sacc.x);
      atomicAdd(dwr + (cb + 1) * KK + k, sacc.y);
      atomicAdd(dwr + (cb + 2) * KK + k, sacc.z);
      atomicAdd(dwr + (cb + 3) * KK + k, sacc.w);
    }
  }
}

// =====================================================================================================
// Stride-2 3x3 depthwise (pad 1) with the input tile in LDS: the downsampling convolutions of the stems and of
// lite_hrnet.py's fuse / transition layers (54 per Lite-HRNet-18 step).  The row-gather kernels they used to take
// (k_dw_fwd / k_dw_bwd_data + k_dw_bwd_weight) ran at a fifth of the traffic-bound time.
// Output tile TH x TW = 4 x 16, 32 channels per block; input tile (2 TH + 1) x (2 TW + 1) with origin (2 oh0 - 1, 2 ow0 - 1).
struct DwS2 {
  static constexpr int TH = 4, TW = 16, XH = 2 * TH + 1, XW = 2 * TW + 1, XPIX = XH * XW, DH = TH + 1, DW = TW + 1, DPIX = DH * DW;
};

// FIN: as in k_dwk_fwd_lds (the pairs in the input tile, the table entries in `red`, both free before the first commit)
template <bool FIN = false>
__global__ void __launch_bounds__(256) k_dws2_fwd_lds(lhn_view x, const float* __restrict__ w, lhn_view y, double* __restrict__ stats,
                                                      int tiles_h, int tiles_w, int cgroups, lhn_bnfin fin, lhn_bnfinsrc fs) {
  using T = DwS2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f4* tx = reinterpret_cast<f4*>(smem);          // [XPIX][8]
  f4* red = tx + T::XPIX * 8;                    // [512]
  f4* wl = red + 512;                            // [9][8]
  const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;
  const int ntile = y.N * tiles_h * tiles_w * cgroups;
  const int cg = blockIdx.x % cgroups;
  const int cvalid = min(8, (x.C - cg * 32) >> 2);          // see k_dwk_fwd_lds
  const bool cok = c4 < cvalid;
  const int c4e = cok ? c4 : 0;
  const int cin = x.coff + cg * 32 + 4 * c4e, cout = y.coff + cg * 32 + 4 * c4e;
  for (int i = tid; i < 72; i += 256) {
    const int k = i >> 3, cc = cg * 32 + 4 * min(i & 7, cvalid - 1);
    wl[i] = (f4){w[(cc + 0) * 9 + k], w[(cc + 1) * 9 + k], w[(cc + 2) * 9 + k], w[(cc + 3) * 9 + k]};
  }
  Xf4 xf;
  if constexpr (FIN) {
    static_assert(T::XPIX * 8 * 16 >= LHN_STAT_REPLICAS * 32 * 16, "the input tile holds the replica pairs of one channel group");
    double* rawd = reinterpret_cast<double*>(tx);
    float* tab = reinterpret_cast<float*>(red);
    const int nc = 4 * cvalid;
    const bool lead = (int)blockIdx.x < cgroups;
    const LhnFinPre pre = lhn_bn_fin_pre(fs, cg * 32, nc, lead);
    double fa[4], fb[4];
    lhn_bn_fin_load<4>(fs.stats, fs.C, cg * 32, nc, fa, fb);
    lhn_bn_fin_put<4>(fa, fb, nc, rawd);
    __syncthreads();
    if (tid < nc) {
      double s1, s2;
      lhn_bn_fin_sum_any(rawd, nc, tid, fs.C, s1, s2);
      lhn_bn_fin_channel(fs, pre, s1, s2, cg * 32, tid, lead, tab, 32);
    }
    __syncthreads();
    xf = lhn_bn_fin_xf(tab, 32, 4 * c4e);
  } else {
    xf = lhn_load_xf(x, cin);
  }
  double sd[4] = {0, 0, 0, 0}, qd[4] = {0, 0, 0, 0};
  constexpr int NIT = (T::XPIX + 31) / 32;
  for (int t = blockIdx.x; t < ntile; t += gridDim.x) {
    int r = t / cgroups;
    const int tw = r % tiles_w;
    r /= tiles_w;
    const int th = r % tiles_h, n = r / tiles_h;
    const int h0 = 2 * th * T::TH - 1, w0 = 2 * tw * T::TW - 1;
    const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (size_t)n * x.cstride + cin) : (f4){1.f, 1.f, 1.f, 1.f};
    const float* xin = x.data + (size_t)n * x.H * x.W * x.cstride + cin;
    f4 raw[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = min(pl + 32 * it, T::XPIX - 1);
      const int ph = i / T::XW, pw = i - ph * T::XW;
      const int ih = min(max(h0 + ph, 0), x.H - 1), iw = min(max(w0 + pw, 0), x.W - 1);
      raw[it] = *reinterpret_cast<const f4*>(xin + ((size_t)ih * x.W + iw) * x.cstride);
    }
    __syncthreads();                 // previous tile consumed (and wl / the resolved table visible)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = pl + 32 * it;
      if (i < T::XPIX) {
        const int ph = i / T::XW, pw = i - ph * T::XW;
        const int ih = h0 + ph, iw = w0 + pw;
        const bool inb = ih >= 0 && ih < x.H && iw >= 0 && iw < x.W;
        tx[i * 8 + c4] = inb ? lhn_apply_xf(raw[it], xf) * gate : (f4){0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();
    f4 s = (f4){0.f, 0.f, 0.f, 0.f}, q = s, kk = s;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = pl + 32 * j, oh = o / T::TW, ow = o - oh * T::TW;
      const int ho = th * T::TH + oh, wo = tw * T::TW + ow;
      if (cok && ho < y.H && wo < y.W) {
        f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) acc += tx[((2 * oh + a) * T::XW + 2 * ow + b) * 8 + c4] * wl[(a * 3 + b) * 8 + c4];
        *reinterpret_cast<f4*>(y.data + ((size_t)(n * y.H + ho) * y.W + wo) * y.cstride + cout) = acc;
        if (cnt == 0) kk = acc;
        const f4 d = acc - kk;
        s += d;
        q += d * d;
        ++cnt;
      }
    }
    lhn_unshift4(sd, qd, s, q, kk, cnt);
  }
  if (stats) {
    const int C = x.C;
    double* st = stats + (size_t)((blockIdx.x / cgroups) % LHN_STAT_REPLICAS) * 2 * C + cg * 32;
    lhn_block_stat_atomics_d(sd, qd, 8, reinterpret_cast<double*>(red), st, st + C, cvalid);
    if (fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block(fin, stats);
  }
}

// fused backward: dx for the 2TH x 2TW input pixels the tile owns (every input pixel belongs to one tile) and dW.
//   dx[ih,iw] = sum over taps (a,b) with (ih+1-a), (iw+1-b) even of dy[(ih+1-a)/2, (iw+1-b)/2] * w[a][b]
//   dW[a][b] += sum over the tile's outputs dy[ho,wo] * x[2ho-1+a, 2wo-1+b]
__global__ void __launch_bounds__(256, 2) k_dws2_bwd_lds(lhn_view x, const float* __restrict__ w, lhn_view y, lhn_gradview gy,
                                                      float* __restrict__ dx, int dx_acc, float* __restrict__ dw, int tiles_h,
                                                      int tiles_w, int cgroups, int nrep, int64_t rep_stride) {
  using T = DwS2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  f4* tx = reinterpret_cast<f4*>(smem);          // [XPIX][8] transformed x (zero outside the image)
  f4* tdy = tx + T::XPIX * 8;                    // [DPIX][8] dy (zero outside the output map); >= 36*8 float4 for the flush
  f4* wl = tdy + T::DPIX * 8;                    // [9][8]
  const int tid = threadIdx.x, c4 = tid & 7, pl = tid >> 3;
  const int ntile = y.N * tiles_h * tiles_w * cgroups;
  const int cg = blockIdx.x % cgroups;
  const int cvalid = min(8, (x.C - cg * 32) >> 2);
  const bool cok = c4 < cvalid;
  const int c4e = cok ? c4 : 0;
  const int cx = x.coff + cg * 32 + 4 * c4e, cy = y.coff + cg * 32 + 4 * c4e;
  const Xf4 xxf = lhn_load_xf(x, cx), yxf = lhn_load_xf(y, cy);
  const Gr4 ygr = lhn_load_coef(gy, y.cstride, cy);
  for (int i = tid; i < 72; i += 256) {
    const int k = i >> 3, cc = cg * 32 + 4 * min(i & 7, cvalid - 1);
    wl[i] = (f4){w[(cc + 0) * 9 + k], w[(cc + 1) * 9 + k], w[(cc + 2) * 9 + k], w[(cc + 3) * 9 + k]};
  }
  f4 accw[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) accw[k] = (f4){0.f, 0.f, 0.f, 0.f};
  constexpr int NITX = (T::XPIX + 31) / 32, NITD = (T::DPIX + 31) / 32;
  for (int t = blockIdx.x; t < ntile; t += gridDim.x) {
    int r = t / cgroups;
    const int tw = r % tiles_w;
    r /= tiles_w;
    const int th = r % tiles_h, n = r / tiles_h;
    const int h0 = 2 * th * T::TH - 1, w0 = 2 * tw * T::TW - 1;       // input tile origin
    const int oh0 = th * T::TH, ow0 = tw * T::TW;                     // dy tile origin
    const f4 xgate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (size_t)n * x.cstride + cx) : (f4){1.f, 1.f, 1.f, 1.f};
    f4 rx[NITX], ry[NITD], rz[NITD];
#pragma unroll
    for (int it = 0; it < NITX; ++it) {
      const int i = min(pl + 32 * it, T::XPIX - 1);
      const int ph = i / T::XW, pw = i - ph * T::XW;
      const int ih = min(max(h0 + ph, 0), x.H - 1), iw = min(max(w0 + pw, 0), x.W - 1);
      rx[it] = *reinterpret_cast<const f4*>(x.data + ((size_t)(n * x.H + ih) * x.W + iw) * x.cstride + cx);
    }
#pragma unroll
    for (int it = 0; it < NITD; ++it) {
      const int i = min(pl + 32 * it, T::DPIX - 1);
      const int ph = i / T::DW, pw = i - ph * T::DW;
      const int ho = min(oh0 + ph, y.H - 1), wo = min(ow0 + pw, y.W - 1);
      const size_t off = ((size_t)(n * y.H + ho) * y.W + wo) * y.cstride + cy;
      ry[it] = *reinterpret_cast<const f4*>(y.data + off);
      rz[it] = *reinterpret_cast<const f4*>(gy.dz + off);
    }
    __syncthreads();                 // previous tile consumed (and wl visible)
#pragma unroll
    for (int it = 0; it < NITX; ++it) {
      const int i = pl + 32 * it;
      if (i < T::XPIX) {
        const int ph = i / T::XW, pw = i - ph * T::XW;
        const int ih = h0 + ph, iw = w0 + pw;
        const bool inb = ih >= 0 && ih < x.H && iw >= 0 && iw < x.W;
        tx[i * 8 + c4] = inb ? lhn_apply_xf(rx[it], xxf) * xgate : (f4){0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int it = 0; it < NITD; ++it) {
      const int i = pl + 32 * it;
      if (i < T::DPIX) {
        const int ph = i / T::DW, pw = i - ph * T::DW;
        const int ho = oh0 + ph, wo = ow0 + pw;
        f4 d = (f4){0.f, 0.f, 0.f, 0.f};
        if (ho < y.H && wo < y.W) {
          const f4 du = lhn_grad_du(y, gy, yxf, ry[it], rz[it], n, ho, wo, cy);
          d = ygr.A * du + ygr.B * ry[it] + ygr.Cc;
        }
        tdy[i * 8 + c4] = d;
      }
    }
    __syncthreads();
    // ---- dW: two outputs per thread
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = pl + 32 * j, oh = o / T::TW, ow = o - oh * T::TW;
      const f4 dyc = tdy[(oh * T::DW + ow) * 8 + c4];          // zero outside the map
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) accw[a * 3 + b] += dyc * tx[((2 * oh + a) * T::XW + 2 * ow + b) * 8 + c4];
    }
    // ---- dx: thread = input column c = pl of the tile (parity fixed), 2 TH rows
    if (dx && cok) {
      const int c = pl, iw = 2 * ow0 + c;
      // column taps: c even -> b = 1 at dy column c/2; c odd -> b = 0 at (c+1)/2 and b = 2 at (c-1)/2
      const int nb = (c & 1) ? 2 : 1;
      const int bA = (c & 1) ? 0 : 1, colA = (c & 1) ? (c + 1) >> 1 : c >> 1, colB = (c - 1) >> 1;
      if (iw < x.W) {
#pragma unroll
        for (int rr = 0; rr < 2 * T::TH; ++rr) {
          const int ih = 2 * oh0 + rr;
          if (ih < x.H) {
            f4 accx = (f4){0.f, 0.f, 0.f, 0.f};
            // row taps: rr even -> a = 1 at dy row rr/2; rr odd -> a = 0 at (rr+1)/2 and a = 2 at (rr-1)/2  (rr is a compile-time constant)
            if ((rr & 1) == 0) {
              const f4* drow = tdy + ((rr >> 1) * T::DW) * 8 + c4;
              accx += drow[colA * 8] * wl[(3 + bA) * 8 + c4];
              if (nb == 2) accx += drow[colB * 8] * wl[(3 + 2) * 8 + c4];
            } else {
              const f4* d0 = tdy + (((rr + 1) >> 1) * T::DW) * 8 + c4;
              const f4* d2 = tdy + (((rr - 1) >> 1) * T::DW) * 8 + c4;
              accx += d0[colA * 8] * wl[(0 + bA) * 8 + c4] + d2[colA * 8] * wl[(6 + bA) * 8 + c4];
              if (nb == 2) accx += d0[colB * 8] * wl[(0 + 2) * 8 + c4] + d2[colB * 8] * wl[(6 + 2) * 8 + c4];
            }
            float* o = dx + ((size_t)(n * x.H + ih) * x.W + iw) * x.cstride + cx;
            if (dx_acc) accx += *reinterpret_cast<const f4*>(o);
            *reinterpret_cast<f4*>(o) = accx;
          }
        }
      }
    }
  }
  // ---- flush dW (as k_dwk_bwd_lds)
  float* dwr = dw + (size_t)((blockIdx.x / cgroups) % nrep) * rep_stride;
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      accw[k].x += __shfl_xor(accw[k].x, o, 64);
      accw[k].y += __shfl_xor(accw[k].y, o, 64);
      accw[k].z += __shfl_xor(accw[k].z, o, 64);
      accw[k].w += __shfl_xor(accw[k].w, o, 64);
    }
  __syncthreads();
  if ((tid & 63) < 8)
#pragma unroll
    for (int k = 0; k < 9; ++k) tdy[(k * 4 + (tid >> 6)) * 8 + c4] = accw[k];
  __syncthreads();
  if (tid < 72) {
    const int k = tid >> 3, cc = tid & 7;
    const f4 sacc = tdy[(k * 4 + 0) * 8 + cc] + tdy[(k * 4 + 1) * 8 + cc] + tdy[(k * 4 + 2) * 8 + cc] + tdy[(k * 4 + 3) * 8 + cc];
    const int cb = cg * 32 + 4 * cc;
    if (cc < cvalid) {
      atomicAdd(dwr + (cb + 0) * 9 + k, sacc.x);
      atomicAdd(dwr + (cb + 1) * 9 + k, sacc.y);
      atomicAdd(dwr + (cb + 2) * 9 + k, sacc.z);
      atomicAdd(dwr + (cb + 3) * 9 + k, sacc.w);
    }
  }
}

// =====================================================================================================
// Launchers: grid, dynamic LDS and arguments of every kernel above.
//
// blocks per XCD when the XCD-aware tile order applies (grid a multiple of 8 and of 8 * cgroups), else 0 = plain order.
// Measured on MI355X (variant B, bs64 256x256): giving each XCD a contiguous run of tiles is SLOWER than the plain
// round-robin order -- forward 3.08 vs 2.93 ms, train step 9.66 vs 9.55 ms: the halo re-reads already hit the Infinity
// Cache, while eight XCDs each streaming one contiguous region load the HBM channels less evenly.  Off unless LHN_XCD_ORDER=1.
static int dw3_xchunk(int grid, int cgroups) {
  static int on = -1;
  if (on < 0) {
    const char* e = getenv("LHN_XCD_ORDER");
    on = (e && e[0] == '1') ? 1 : 0;
  }
  return (on && grid % (8 * cgroups) == 0) ? grid / 8 : 0;
}
static int dw3_grid(int ntile, int cgroups, int per_cu) {
  int g = lhn_num_cus() * per_cu;
  g -= g % cgroups;
  if (g > ntile) g = ntile;       // ntile is a multiple of cgroups
  if (g < cgroups) g = cgroups;
  return g;
}

template <int K, int DIL, int NS = 1, bool FIN = false>
static void launch_dwk_fwd(const lhn_view* x, const float* w, const lhn_view* y, double* stats, lhn_bnfin fin, hipStream_t s, int ps = 1,
                           const DwExtra* exp = nullptr, const lhn_bnfinsrc* fsp = nullptr) {
  DwExtra ex;
  if (exp) ex = *exp; else { ex.n = 0; ex.sum_out = nullptr; }
  lhn_bnfinsrc fs;
  if (FIN && fsp) fs = *fsp; else memset(&fs, 0, sizeof(fs));
  constexpr int TH = 8, TW = 32, P = DIL * (K - 1) / 2;
  const int cg = (x->C + 31) / 32;
  const int sh = (y->H + ps - 1) / ps, sw = (y->W + ps - 1) / ps;       // largest parity sub-lattice
  const int th = (sh + TH - 1) / TH, tw = (sw + TW - 1) / TW, ntile = y->N * ps * ps * th * tw * cg;
  const size_t lds = (size_t)((TH + 2 * P) * (TW + 2 * P) * 8 + 512 + K * K * 8) * 16;
  const int per_cu = lds > 80 * 1024 ? 1 : (lds > 52 * 1024 ? 2 : 3);
  static LhnKernelCfg cfg;
  int resident = 2;
  (void)lhn_kernel_cfg(cfg, &k_dwk_fwd_lds<K, DIL, NS, FIN>, lds, 4, &resident);
  // (2 / 3 / 4 / 8 / 16 blocks per CU measured in round 3: forward 2.65 / 2.68 / 2.66 / 2.71 / 2.71 ms).  FIN: one round of resident
  // workgroups -- every workgroup pays the prologue fold once, and six per CU with two resident paid it three times in a row
  // (64 x 64 x 64 channels at batch 64: 33.6 -> 48 us, against 39 us with the separate launch)
  const int grid = dw3_grid(ntile, cg, FIN ? resident : per_cu * 2);
  hipLaunchKernelGGL((k_dwk_fwd_lds<K, DIL, NS, FIN>), dim3(grid), dim3(256), lds, s, *x, w, *y, stats, th, tw, cg, fin, ps, ex,
                     dw3_xchunk(grid, cg), fs);
}
template <int K, int DIL, bool BNS = false, bool FOLD = false>
static void launch_dwk_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_acc,
                           float* dw, int nrep, int64_t rep_stride, hipStream_t s, int ps = 1, const DwBnSum* bsp = nullptr,
                           const lhn_bnbwdsrc* fsp = nullptr) {
  constexpr int TH = 8, TW = 16, P = DIL * (K - 1) / 2;
  DwBnSum bs;
  if (bsp) bs = *bsp; else { bs.sums = nullptr; bs.save = nullptr; bs.C = bs.coff = 0; bs.add[0] = bs.add[1] = nullptr; }
  lhn_bnbwdsrc fs;
  if (FOLD && fsp) fs = *fsp; else memset(&fs, 0, sizeof(fs));
  const int cg = (x->C + 31) / 32;
  const int sh = (x->H + ps - 1) / ps, sw = (x->W + ps - 1) / ps;
  const int th = (sh + TH - 1) / TH, tw = (sw + TW - 1) / TW, ntile = x->N * ps * ps * th * tw * cg;
  const size_t lds = (size_t)((TH + 2 * P) * (TW + 2 * P) * 16 + 256 + 2 * K * K * 8 + (BNS ? TH * TW * 8 + 16 : 0) + (FOLD ? 24 : 0)) * 16;
  static LhnKernelCfg cfg;
  (void)lhn_kernel_cfg(cfg, &k_dwk_bwd_lds<K, DIL, BNS, FOLD>, lds, 4, nullptr);
  const int grid = dw3_grid(ntile, cg, 4);
  hipLaunchKernelGGL((k_dwk_bwd_lds<K, DIL, BNS, FOLD>), dim3(grid), dim3(256), lds, s, *x, w, *y, *gy, dx, dx_acc, dw, th, tw,
                     cg, nrep, rep_stride, ps, bs, dw3_xchunk(grid, cg), fs);
}
template <int DIL, bool BNS = false>
static void launch_dw3_bwd_rows(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_acc,
                                float* dw, int nrep, int64_t rep_stride, hipStream_t s, int ps = 1, const DwBnSum* bsp = nullptr,
                                const lhn_bnbwdsrc* fsp = nullptr) {
  constexpr int P = DIL, R = 2 * P + 2, WW = 32 + 2 * P;
  DwBnSum bs;
  if (bsp) bs = *bsp; else { bs.sums = nullptr; bs.save = nullptr; bs.C = bs.coff = 0; bs.add[0] = bs.add[1] = nullptr; }
  lhn_bnbwdsrc fs;      // the fold's scratch is 16 KB of the dy ring (17,408 B at DIL = 1)
  if (fsp) fs = *fsp; else memset(&fs, 0, sizeof(fs));
  static_assert(R * WW * 8 * 16 >= 2 * LHN_FIN_THREADS * 8, "dy ring holds the replica fold's partials");
  const int cg = (x->C + 31) / 32;
  const int sh = (x->H + ps - 1) / ps, sw = (x->W + ps - 1) / ps;     // largest parity sub-lattice
  const int nstrips = (sw + 31) / 32;
  const size_t lds = (size_t)(2 * R * WW * 8 + 2 * 9 * 8 + 16 + (BNS ? R * 32 * 8 : 0)) * 16;
  static LhnKernelCfg cfg;
  int per_cu = 1;
  (void)lhn_kernel_cfg(cfg, &k_dw3_bwd_rows<DIL, BNS>, lds, 8, &per_cu);
  // row chunks: about one item per resident workgroup, at least 8 rows each (the 2*P halo rows are loaded once per item)
  const int base = x->N * ps * ps * nstrips * cg;
  int nch = (lhn_num_cus() * per_cu + base - 1) / base;
  nch = std::max(1, std::min(nch, (sh + 7) / 8));
  const int CH = (sh + nch - 1) / nch;
  nch = (sh + CH - 1) / CH;
  const int ntile = base * nch;
  const int grid = dw3_grid(ntile, cg, per_cu);       // one round of resident workgroups
  hipLaunchKernelGGL((k_dw3_bwd_rows<DIL, BNS>), dim3(grid), dim3(256), lds, s, *x, w, *y, *gy, dx, dx_acc, dw, nstrips, nch, CH, cg,
                     nrep, rep_stride, ps, bs, fs);
}
// returns 1 if the stride-2 tiled kernel was launched
template <bool FIN = false>
static int dws2_fwd(const lhn_view* x, const float* w, const lhn_view* y, double* stats, lhn_bnfin fin, hipStream_t s,
                    const lhn_bnfinsrc* fsp = nullptr) {
  using T = DwS2;
  lhn_bnfinsrc fs;
  if (FIN && fsp) fs = *fsp; else memset(&fs, 0, sizeof(fs));
  const int cg = (x->C + 31) / 32;
  const int th = (y->H + T::TH - 1) / T::TH, tw = (y->W + T::TW - 1) / T::TW, ntile = y->N * th * tw * cg;
  size_t lds = (size_t)(T::XPIX * 8 + 512 + 72) * 16;
  static LhnKernelCfg cfg;
  int resident = 3;
  if (!lhn_kernel_cfg(cfg, &k_dws2_fwd_lds<FIN>, lds, 4, &resident)) return 0;
  // (FIN: one round of resident workgroups, see launch_dwk_fwd)
  hipLaunchKernelGGL(k_dws2_fwd_lds<FIN>, dim3(dw3_grid(ntile, cg, FIN ? resident : 6)), dim3(256), lds, s, *x, w, *y, stats, th, tw, cg, fin, fs);
  return 1;
}
static int dws2_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_acc, float* dw,
                    int nrep, int64_t rep_stride, hipStream_t s) {
  using T = DwS2;
  const int cg = (x->C + 31) / 32;
  const int th = (y->H + T::TH - 1) / T::TH, tw = (y->W + T::TW - 1) / T::TW, ntile = y->N * th * tw * cg;
  const size_t lds = (size_t)((T::XPIX + T::DPIX) * 8 + 72) * 16;
  static LhnKernelCfg cfg;
  if (!lhn_kernel_cfg(cfg, &k_dws2_bwd_lds, lds, 4, nullptr)) return 0;
  hipLaunchKernelGGL(k_dws2_bwd_lds, dim3(dw3_grid(ntile, cg, 4)), dim3(256), lds, s, *x, w, *y, *gy, dx, dx_acc, dw, th, tw, cg, nrep, rep_stride);
  return 1;
}
// the row-gather kernels: any k, stride, padding and dilation
template <int K>
static void launch_dw_fwd_gather(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int stride, int pad, int dil,
                                 lhn_bnfin fin, hipStream_t s) {
  const size_t lds = (size_t)(K * K * x->C) * 4 + 256 * 2 * 16;
  const int grid = grid_for((int64_t)y->N * y->H, 1, 8);
  hipLaunchKernelGGL((k_dw_fwd<K>), dim3(grid), dim3(256), lds, s, *x, w, *y, stats, stride, pad, dil, fin, 0);
}
// data gradient unless dx is NULL, then the weight gradient unless dw is NULL (identity depthwise: no weight to learn), KR kernel
// rows per launch
template <int K, int KR>
static void launch_dw_bwd_gather(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_acc,
                                 float* dw, int stride, int pad, int dil, int nrep, int64_t rep_stride, hipStream_t s) {
  if (dx) {
    const size_t lds = (size_t)(K * K * x->C) * 4;
    const int g = grid_for((int64_t)x->N * x->H, 1, 8);
    hipLaunchKernelGGL((k_dw_bwd_data<K>), dim3(g), dim3(256), lds, s, *x, w, *y, *gy, dx, dx_acc, stride, pad, dil);
  }
  const int gw = grid_for((int64_t)y->N * y->H, 1, 4);
  for (int kh = 0; dw && kh < K; kh += KR)
    hipLaunchKernelGGL((k_dw_bwd_weight<K, KR>), dim3(gw), dim3(256), 0, s, *x, *y, *gy, dw, stride, pad, dil, kh, nrep, rep_stride);
}

// =====================================================================================================
// Route: which kernel a depthwise call runs.  dw_fwd_route() and dw_bwd_route() are pure and the only place that knows the rules;
// the dispatchers below and lhn_conv_dw_route() (the host-only query, which the tests and profiles/dw_instances.md read) call them.
struct DwShape {
  int H, W, C;                  // of x
  int k, stride, pad, dil;
  unsigned f;                   // LHN_DW_F_*: what the call carries
};
enum DwKern {
  DW_NONE = 0,      // no kernel for this k / dilation with these features
  DW_NARROW,        // none either: the features live in the tiled stride-1 kernels, which this geometry does not reach
  DWF_LDS31, DWF_LDS32, DWF_LDS71, DWF_LDS31_NS2, DWF_S2, DWF_LDS31_FIN, DWF_S2_FIN, DWF_GATHER1, DWF_GATHER3, DWF_GATHER5, DWF_GATHER7,
  DWB_ROWS1, DWB_ROWS1_BNS, DWB_ROWS2, DWB_LDS31, DWB_LDS31_BNS, DWB_LDS31_FOLD, DWB_LDS31_BNS_FOLD, DWB_LDS32, DWB_LDS71, DWB_S2,
  DWB_GATHER1, DWB_GATHER3, DWB_GATHER7
};
struct DwRoute {
  DwKern kern;
  int ps;                       // 2: a dilation-2 convolution run as four dilation-1 convolutions on the parity sub-lattices
  bool separate_finalize;       // a finalize source is present and the kernel does not take it in its prologue (forward: lhn_bnfinsrc
                                // and lhn_bn_finalize in front; backward: lhn_bnbwdsrc and lhn_bn_bwd_finalize2)
};

// LHN_DW_SW_*, read from the environment once.  LHN_DW_GATHER=1: the row-gather kernels.  LHN_DW_BWD_V1=1: the 3x3 backward runs the
// 8 x 16 tile kernel k_dwk_bwd_lds instead of k_dw3_bwd_rows.  LHN_DW_BWD_SMALL=0: no small-map route, for A/B runs.
static unsigned dw_switches() {
  static int v = -1;
  if (v < 0) {
    const char *v1 = getenv("LHN_DW_BWD_V1"), *sm = getenv("LHN_DW_BWD_SMALL");
    v = (lhn_dw_force_gather() ? LHN_DW_SW_GATHER : 0) | ((v1 && v1[0] == '1') ? LHN_DW_SW_BWD_V1 : 0) |
        ((sm && sm[0] == '0') ? 0 : LHN_DW_SW_BWD_SMALL);
  }
  return (unsigned)v;
}

// The tiled kernels are built for stride 1 with "same" padding on maps at least 8 wide: 3x3 at dilation 1 and 2 (W >= 16: on the
// parity sub-lattices of the dilation-1 kernel) and 7x7; 3x3 / stride 2 / pad 1 has a tiled kernel of its own.
static bool dw_tiled_geometry(const DwShape& s) { return s.stride == 1 && s.pad == s.dil * (s.k - 1) / 2 && s.W >= 8; }
static int dw_parity_split(const DwShape& s) { return (s.k == 3 && s.dil == 2 && s.W >= 16) ? 2 : 1; }

// A finalize source (LHN_DW_F_FINSRC) rides in the 3x3 / dilation 1 / stride 1 tile kernel and in the stride-2 one; every other
// kernel gets the lhn_bn_finalize launch in front.
static DwRoute dw_fwd_route(const DwShape& s, unsigned sw) {
  const bool tiled = dw_tiled_geometry(s), fs = s.f & LHN_DW_F_FINSRC;
  const int ps = dw_parity_split(s);
  if (s.f & LHN_DW_F_EXTRA)      // two summed sources (MSRB's second round): 3x3 on the dilation-1 kernel only; ignores LHN_DW_GATHER
    return {(tiled && s.k == 3 && (s.dil == 1 || ps == 2)) ? DWF_LDS31_NS2 : DW_NONE, ps, fs};
  if (!(s.f & LHN_DW_F_NO_WEIGHT) && !(sw & LHN_DW_SW_GATHER)) {
    if (tiled && s.k == 3 && s.dil == 1 && fs) return {DWF_LDS31_FIN, 1, false};
    if (tiled && s.k == 3 && (s.dil == 1 || ps == 2)) return {DWF_LDS31, ps, fs};
    if (tiled && s.k == 3 && s.dil == 2) return {DWF_LDS32, 1, fs};
    if (tiled && s.k == 7 && s.dil == 1) return {DWF_LDS71, 1, fs};
    if (s.k == 3 && s.stride == 2 && s.pad == 1 && s.dil == 1) return {fs ? DWF_S2_FIN : DWF_S2, 1, false};
  }
  return {s.k == 1 ? DWF_GATHER1 : s.k == 3 ? DWF_GATHER3 : s.k == 5 ? DWF_GATHER5 : s.k == 7 ? DWF_GATHER7 : DW_NONE, 1, fs};
}

// The small-map rule (3x3, dilation 1): H * W <= 256 pixels run the 8 x 16 tile kernel, whose whole halo tile is ONE batch of loads,
// where a row strip pays CH + 2 = 10 dependent memory latencies and a barrier per row whatever the map size.  Train step of variant B
// at batch 64, per launch, rows kernel against the tile kernel with its separate finalize launch (profiles/dwsmall_launches.md): 8^2
// 21.8 us against 10.9 + 4.7, 16^2 24.2 against 14.0 + 4.8, 32^2 30.3 against 31.7 + 4.9 -- so 32^2 and everything between 16^2 and
// 32^2, which was not measured, stay on k_dw3_bwd_rows, where 64^2 and 128^2 were tuned.  The route's instances are the FOLD ones
// (they take the finalize in their prologue as the row kernel does), also when the call has no finalize source.
static DwRoute dw_bwd_route(const DwShape& s, unsigned sw) {
  const bool bns = s.f & LHN_DW_F_BNSUM, ext = s.f & (LHN_DW_F_BNSUM | LHN_DW_F_ADDS);     // ext: these ignore LHN_DW_GATHER
  const bool v1 = sw & LHN_DW_SW_BWD_V1;
  const bool small = (sw & LHN_DW_SW_BWD_SMALL) && s.k == 3 && s.dil == 1 && (int64_t)s.H * s.W <= 256;
  const int ps = dw_parity_split(s);
  DwRoute r = {DW_NONE, 1, false};
  if (!(s.f & LHN_DW_F_NO_WEIGHT) && dw_tiled_geometry(s) && (ext || !(sw & LHN_DW_SW_GATHER))) {
    if (bns) {       // the producer's BatchNorm sums: 3x3 / dilation 1 instances only, dx stored
      if (s.k == 3 && s.dil == 1 && !(s.f & (LHN_DW_F_NO_DX | LHN_DW_F_DX_ACC)))
        r.kern = v1 ? DWB_LDS31_BNS : small ? DWB_LDS31_BNS_FOLD : DWB_ROWS1_BNS;
    } else if (s.k == 3 && (s.dil == 1 || ps == 2)) {
      r.kern = v1 ? DWB_LDS31 : small ? DWB_LDS31_FOLD : DWB_ROWS1;
      r.ps = ps;
    } else if (s.k == 3 && s.dil == 2) {
      r.kern = v1 ? DWB_LDS32 : DWB_ROWS2;
    } else if (s.k == 7 && s.dil == 1) {
      r.kern = DWB_LDS71;      // K = 7: the tile kernel, which never folds
    }
  } else if (ext) {
    r.kern = DW_NARROW;
  }
  if (r.kern == DW_NONE && !ext) {
    if (!(s.f & LHN_DW_F_NO_WEIGHT) && s.k == 3 && s.stride == 2 && s.pad == 1 && s.dil == 1 && !(sw & LHN_DW_SW_GATHER)) r.kern = DWB_S2;
    else r.kern = s.k == 1 ? DWB_GATHER1 : s.k == 3 ? DWB_GATHER3 : s.k == 7 ? DWB_GATHER7 : DW_NONE;
  }
  const bool folds = r.kern == DWB_ROWS1 || r.kern == DWB_ROWS1_BNS || r.kern == DWB_ROWS2 || r.kern == DWB_LDS31_FOLD ||
                     r.kern == DWB_LDS31_BNS_FOLD;
  r.separate_finalize = (s.f & LHN_DW_F_FIN) && !folds;
  return r;
}

// =====================================================================================================
// Dispatchers: validate once, ask the route, issue the separate finalize launch when the route says so, launch.
static int dw_fwd_finalize(const lhn_bnfinsrc* f, void* stream) {
  return lhn_bn_finalize(f->stats, f->gamma, f->beta, f->running_mean, f->running_var, f->num_batches_tracked, f->table, f->cstride, f->coff,
                         f->C, f->save_mean_invstd, f->count, f->eps, f->momentum, f->slope, 1, f->conv_bias, stream);
}
static int dw_fwd_run(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int k, int stride, int pad, int dil,
                      const lhn_bnfin* finp, const lhn_view* extra, const float* coef2, const lhn_view* sum_out, const lhn_bnfinsrc* fsrc,
                      void* stream) {
  lhn_bnfin fin;
  if (finp && stats) fin = *finp; else fin.counter = nullptr;
  if (fsrc && !fsrc->stats) fsrc = nullptr;
  if (fsrc)
    LHN_CHECK_ARG(lhn_view_ok(x) && !extra && fsrc->table && fsrc->table == x->table && fsrc->cstride == x->cstride && fsrc->coff == x->coff &&
                      fsrc->C == x->C && fsrc->count >= 1 && (!fsrc->running_mean || fsrc->running_var),
                  "lhn_conv_dw_fwd: the finalize source must be the BatchNorm of x (its table and channel slice), one source");
  if (!extra) {
    LHN_CHECK_ARG(!sum_out, "lhn_conv_dw_fwd: sum_out without a second source");
    LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && (w || k == 1), "lhn_conv_dw_fwd: bad view / null pointer (w may be NULL = ones only for k=1)");
    LHN_CHECK_ARG(x->C == y->C && x->C % 4 == 0 && x->C <= 512, "lhn_conv_dw_fwd: channels %d -> %d (multiple of 4, <= 512)", x->C, y->C);
    LHN_CHECK_ARG((k == 1 || k == 3 || k == 5 || k == 7) && stride >= 1 && dil >= 1 && pad >= 0, "lhn_conv_dw_fwd: k=%d stride=%d dil=%d", k, stride, dil);
    const int Ho = (x->H + 2 * pad - dil * (k - 1) - 1) / stride + 1, Wo = (x->W + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    LHN_CHECK_ARG(y->N == x->N && y->H == Ho && y->W == Wo, "lhn_conv_dw_fwd: output %dx%d, expected %dx%d", y->H, y->W, Ho, Wo);
    LHN_CHECK_ARG(lhn_no_pend(x), "lhn_conv_dw_fwd: lhn_view.pend is reserved (NULL)");
  } else {
    LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && lhn_view_ok(extra) && w && coef2, "lhn_conv_dw_fwd: bad view / null pointer");
    LHN_CHECK_ARG(extra->C == x->C && extra->N == x->N && extra->H == x->H && extra->W == x->W, "lhn_conv_dw_fwd: extra source geometry");
    LHN_CHECK_ARG(x->C == y->C && y->N == x->N && y->H == x->H && y->W == x->W, "lhn_conv_dw_fwd: same-size output");
    LHN_CHECK_ARG(!sum_out || (sum_out->data && sum_out->C == x->C && sum_out->N == x->N && sum_out->H == x->H && sum_out->W == x->W &&
                               sum_out->cstride % 4 == 0 && sum_out->coff % 4 == 0 && sum_out->coff + sum_out->C <= sum_out->cstride),
                  "lhn_conv_dw_fwd: sum_out geometry (same pixels and channels as x)");
  }
  const DwShape sh = {x->H, x->W, x->C, k, stride, pad, dil,
                      (w ? 0u : LHN_DW_F_NO_WEIGHT) | (extra ? LHN_DW_F_EXTRA : 0u) | (fsrc ? LHN_DW_F_FINSRC : 0u)};
  const DwRoute r = dw_fwd_route(sh, dw_switches());
  LHN_CHECK_ARG(!extra || (r.kern != DW_NONE && lhn_no_pend(x) && lhn_no_pend(extra)),
                "lhn_conv_dw_fwd: a second source needs k=3, stride 1, 'same' padding, W >= 8 (got k=%d s=%d C=%d W=%d)", k, stride, x->C, y->W);
  DwExtra ex;
  memset(&ex, 0, sizeof(ex));
  if (extra) {
    ex.v = *extra;
    ex.coef[0] = coef2[0];
    ex.coef[1] = coef2[1];
    ex.n = 1;
    ex.sum_out = sum_out ? sum_out->data : nullptr;
    ex.so_cstride = sum_out ? sum_out->cstride : 0;
    ex.so_coff = sum_out ? sum_out->coff : 0;
  }
  hipStream_t s = (hipStream_t)stream;
  if (r.separate_finalize && r.kern != DW_NONE) {
    const int rc = dw_fwd_finalize(fsrc, stream);
    if (rc) return rc;
  }
  switch (r.kern) {
    case DWF_LDS31_FIN: launch_dwk_fwd<3, 1, 1, true>(x, w, y, stats, fin, s, 1, &ex, fsrc); break;
    case DWF_S2_FIN: {
      if (dws2_fwd<true>(x, w, y, stats, fin, s, fsrc)) break;
      const int rc = dw_fwd_finalize(fsrc, stream);      // (its LDS reservation was refused: the launch in front, then the gather kernel)
      if (rc) return rc;
      launch_dw_fwd_gather<3>(x, w, y, stats, stride, pad, dil, fin, s);
      break;
    }
    case DWF_LDS31: launch_dwk_fwd<3, 1>(x, w, y, stats, fin, s, r.ps, &ex); break;
    case DWF_LDS32: launch_dwk_fwd<3, 2>(x, w, y, stats, fin, s, 1, &ex); break;
    case DWF_LDS71: launch_dwk_fwd<7, 1>(x, w, y, stats, fin, s, 1, &ex); break;
    case DWF_LDS31_NS2: launch_dwk_fwd<3, 1, 2>(x, w, y, stats, fin, s, r.ps, &ex); break;
    case DWF_S2:
      if (dws2_fwd(x, w, y, stats, fin, s)) break;
      [[fallthrough]];      // (its LDS reservation was refused: the gather kernel computes the same)
    case DWF_GATHER3: launch_dw_fwd_gather<3>(x, w, y, stats, stride, pad, dil, fin, s); break;
    case DWF_GATHER1: launch_dw_fwd_gather<1>(x, w, y, stats, stride, pad, dil, fin, s); break;
    case DWF_GATHER5: launch_dw_fwd_gather<5>(x, w, y, stats, stride, pad, dil, fin, s); break;
    case DWF_GATHER7: launch_dw_fwd_gather<7>(x, w, y, stats, stride, pad, dil, fin, s); break;
    default: LHN_CHECK_ARG(false, "lhn_conv_dw_fwd: no kernel for k=%d", k);
  }
  LHN_CHECK_LAUNCH("lhn_conv_dw_fwd");
  return 0;
}

static int dw_bwd_run(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate, float* dw,
                      int k, int stride, int pad, int dil, int nrep, int64_t rep_stride, const lhn_bnsum* bns, const float* dx_add0,
                      const float* dx_add1, const lhn_bnbwdsrc* fin, void* stream) {
  if (nrep < 1) nrep = 1;
  if (bns && !bns->sums) bns = nullptr;
  if (fin && !fin->sums) fin = nullptr;
  const bool has_add = dx_add0 || dx_add1;
  const bool same = stride == 1 && pad == dil * (k - 1) / 2;
  LHN_CHECK_ARG(!(bns && has_add), "lhn_conv_dw_bwd: producer sums and gradient addends exclude each other");
  if (fin)
    LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && gy && gy->dz && gy->coef && fin->save_mean_invstd && fin->count > 0 &&
                      fin->stat_channels >= y->C && x->C == y->C && lhn_no_pend(x) && lhn_no_pend(y),
                  "lhn_conv_dw_bwd: finalize source needs gy->coef, saved statistics and stat_channels >= C");
  if (bns) {
    LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && gy && gy->dz && w && dw && dx && bns->save && lhn_no_pend(x) && lhn_no_pend(y),
                  "lhn_conv_dw_bwd: bad view / null pointer");
    LHN_CHECK_ARG(!dx_accumulate && !x->gate && same && x->C % 32 == 0 && x->C == y->C && bns->coff >= 0 && bns->coff + x->C <= bns->C,
                  "lhn_conv_dw_bwd: fused BatchNorm sums need this convolution to be the only, ungated, stride-1 reader of x (dx stored)");
  } else if (has_add) {
    LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && gy && gy->dz && w && dw && dx && lhn_no_pend(x) && lhn_no_pend(y),
                  "lhn_conv_dw_bwd: bad view / null pointer");
    LHN_CHECK_ARG(same && x->C == y->C, "lhn_conv_dw_bwd: gradient addends need the tiled stride-1 kernel (W >= 8)");
  } else {
    LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && gy && gy->dz && ((w && dw) || k == 1) && lhn_no_pend(x) && lhn_no_pend(y),
                  "lhn_conv_dw_bwd: bad view / null pointer");
    LHN_CHECK_ARG(x->C == y->C && x->C % 4 == 0 && x->C <= 512, "lhn_conv_dw_bwd: channels");
    LHN_CHECK_ARG(k == 1 || k == 3 || k == 7, "lhn_conv_dw_bwd: k=%d (1, 3 or 7)", k);
  }
  const DwShape sh = {x->H, x->W, x->C, k, stride, pad, dil,
                      ((w && dw) ? 0u : LHN_DW_F_NO_WEIGHT) | (bns ? LHN_DW_F_BNSUM : 0u) | (has_add ? LHN_DW_F_ADDS : 0u) |
                          (fin ? LHN_DW_F_FIN : 0u) | (dx ? 0u : LHN_DW_F_NO_DX) | (dx_accumulate ? LHN_DW_F_DX_ACC : 0u)};
  const DwRoute r = dw_bwd_route(sh, dw_switches());
  if (bns) {
    LHN_CHECK_ARG(r.kern != DW_NARROW,
                  "lhn_conv_dw_bwd: fused BatchNorm sums need this convolution to be the only, ungated, stride-1 reader of x (dx stored)");
    LHN_CHECK_ARG(r.kern != DW_NONE, "lhn_conv_dw_bwd: fused BatchNorm sums are built for the 3x3 / dilation 1 kernel (k=%d dil=%d)", k, dil);
  } else if (has_add) {
    LHN_CHECK_ARG(r.kern != DW_NARROW, "lhn_conv_dw_bwd: gradient addends need the tiled stride-1 kernel (W >= 8)");
    LHN_CHECK_ARG(r.kern != DW_NONE, "lhn_conv_dw_bwd: no tiled kernel for k=%d dil=%d", k, dil);
  }
  // (a finalize that rides in the kernel: the plain call's channel limit, whatever else the call carries)
  LHN_CHECK_ARG(!fin || r.separate_finalize || x->C <= 512, "lhn_conv_dw_bwd: channels");
  if (r.separate_finalize) {
    const int rc = lhn_bn_bwd_finalize2(fin->sums, fin->gamma, fin->save_mean_invstd, const_cast<float*>(gy->coef), y->cstride, y->coff,
                                        y->C, fin->stat_channels, fin->count, fin->dgamma, fin->dbeta, fin->pgrad_scale, stream);
    if (rc) return rc;
  }
  const DwBnSum bs = {bns ? bns->sums : nullptr, bns ? bns->save : nullptr, bns ? bns->C : 0, bns ? bns->coff : 0,
                      {dx_add0 ? dx_add0 : dx_add1, dx_add0 ? dx_add1 : nullptr}};
  const lhn_bnbwdsrc* fs = r.separate_finalize ? nullptr : fin;
  const int acc = bns ? 0 : dx_accumulate;
  hipStream_t s = (hipStream_t)stream;
  switch (r.kern) {
    case DWB_ROWS1: launch_dw3_bwd_rows<1>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, r.ps, &bs, fs); break;
    case DWB_ROWS1_BNS: launch_dw3_bwd_rows<1, true>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, 1, &bs, fs); break;
    case DWB_ROWS2: launch_dw3_bwd_rows<2>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, 1, &bs, fs); break;
    case DWB_LDS31: launch_dwk_bwd<3, 1>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, r.ps, &bs); break;
    case DWB_LDS31_BNS: launch_dwk_bwd<3, 1, true>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, 1, &bs); break;
    case DWB_LDS31_FOLD: launch_dwk_bwd<3, 1, false, true>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, 1, &bs, fs); break;
    case DWB_LDS31_BNS_FOLD: launch_dwk_bwd<3, 1, true, true>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, 1, &bs, fs); break;
    case DWB_LDS32: launch_dwk_bwd<3, 2>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, 1, &bs); break;
    case DWB_LDS71: launch_dwk_bwd<7, 1>(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s, 1, &bs); break;
    case DWB_S2:
      if (dws2_bwd(x, w, y, gy, dx, acc, dw, nrep, rep_stride, s)) break;
      [[fallthrough]];      // (its LDS reservation was refused: the gather pair computes the same)
    case DWB_GATHER3: launch_dw_bwd_gather<3, 3>(x, w, y, gy, dx, acc, dw, stride, pad, dil, nrep, rep_stride, s); break;
    case DWB_GATHER1: launch_dw_bwd_gather<1, 1>(x, w, y, gy, dx, acc, dw, stride, pad, dil, nrep, rep_stride, s); break;
    case DWB_GATHER7: launch_dw_bwd_gather<7, 1>(x, w, y, gy, dx, acc, dw, stride, pad, dil, nrep, rep_stride, s); break;
    default: LHN_CHECK_ARG(false, "lhn_conv_dw_bwd: no kernel for k=%d", k);
  }
  LHN_CHECK_LAUNCH("lhn_conv_dw_bwd");
  return 0;
}

// =====================================================================================================
// Entry points.  The numbered forms differ in what a call may carry; each forwards to the widest.
extern "C" int lhn_conv_dw_fwd(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int k, int stride,
                               int pad, int dil, const lhn_bnfin* finp, void* stream) {
  return lhn_conv_dw_fwd3(x, w, y, stats, k, stride, pad, dil, finp, nullptr, nullptr, nullptr, stream);
}
extern "C" int lhn_conv_dw_fwd2(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int k, int stride,
                                int pad, int dil, const lhn_bnfin* finp, const lhn_view* extra, const float* coef2, void* stream) {
  return lhn_conv_dw_fwd3(x, w, y, stats, k, stride, pad, dil, finp, extra, coef2, nullptr, stream);
}
extern "C" int lhn_conv_dw_fwd3(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int k, int stride,
                                int pad, int dil, const lhn_bnfin* finp, const lhn_view* extra, const float* coef2,
                                const lhn_view* sum_out, void* stream) {
  return dw_fwd_run(x, w, y, stats, k, stride, pad, dil, finp, extra, coef2, sum_out, nullptr, stream);
}
extern "C" int lhn_conv_dw_fwd4(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int k, int stride,
                                int pad, int dil, const lhn_bnfin* finp, const lhn_view* extra, const float* coef2,
                                const lhn_view* sum_out, const lhn_bnfinsrc* finsrc, void* stream) {
  return dw_fwd_run(x, w, y, stats, k, stride, pad, dil, finp, extra, coef2, sum_out, finsrc, stream);
}

extern "C" int lhn_conv_dw_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                               int dx_accumulate, float* dw, int k, int stride, int pad, int dil, int nrep, int64_t rep_stride,
                               void* stream) {
  return lhn_conv_dw_bwd4(x, w, y, gy, dx, dx_accumulate, dw, k, stride, pad, dil, nrep, rep_stride, nullptr, nullptr, nullptr, nullptr, stream);
}
extern "C" int lhn_conv_dw_bwd2(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, int k, int stride, int pad, int dil, int nrep, int64_t rep_stride,
                                double* bn_sums, const float* bn_save, int bn_C, int bn_coff, void* stream) {
  const lhn_bnsum bns = {bn_sums, bn_save, bn_C, bn_coff};
  return lhn_conv_dw_bwd4(x, w, y, gy, dx, dx_accumulate, dw, k, stride, pad, dil, nrep, rep_stride, &bns, nullptr, nullptr, nullptr, stream);
}
extern "C" int lhn_conv_dw_bwd3(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, int k, int stride, int pad, int dil, int nrep, int64_t rep_stride,
                                const float* dx_add0, const float* dx_add1, void* stream) {
  return lhn_conv_dw_bwd4(x, w, y, gy, dx, dx_accumulate, dw, k, stride, pad, dil, nrep, rep_stride, nullptr, dx_add0, dx_add1, nullptr, stream);
}
extern "C" int lhn_conv_dw_bwd4(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, int k, int stride, int pad, int dil, int nrep, int64_t rep_stride,
                                const lhn_bnsum* bns, const float* dx_add0, const float* dx_add1, const lhn_bnbwdsrc* fin,
                                void* stream) {
  return dw_bwd_run(x, w, y, gy, dx, dx_accumulate, dw, k, stride, pad, dil, nrep, rep_stride, bns, dx_add0, dx_add1, fin, stream);
}

// Host only: the name of what dw_fwd_run / dw_bwd_run would launch (include/lhn.h).
extern "C" const char* lhn_conv_dw_route(int backward, int H, int W, int C, int k, int stride, int pad, int dil, int features,
                                         int switches) {
  static const char* const name[] = {
      nullptr, nullptr, "k_dwk_fwd_lds<3,1>", "k_dwk_fwd_lds<3,2>", "k_dwk_fwd_lds<7,1>", "k_dwk_fwd_lds<3,1,2>", "k_dws2_fwd_lds",
      "k_dwk_fwd_lds<3,1,1,true>", "k_dws2_fwd_lds<true>", "k_dw_fwd<1>", "k_dw_fwd<3>", "k_dw_fwd<5>", "k_dw_fwd<7>",
      "k_dw3_bwd_rows<1>", "k_dw3_bwd_rows<1,BNS>", "k_dw3_bwd_rows<2>", "k_dwk_bwd_lds<3,1>", "k_dwk_bwd_lds<3,1,BNS>",
      "k_dwk_bwd_lds<3,1,false,true>", "k_dwk_bwd_lds<3,1,BNS,true>", "k_dwk_bwd_lds<3,2>", "k_dwk_bwd_lds<7,1>", "k_dws2_bwd_lds"};
  static const char* const gdata[] = {"k_dw_bwd_data<1>", "k_dw_bwd_data<3>", "k_dw_bwd_data<7>"};
  static const char* const gweight[] = {"k_dw_bwd_weight<1,1>", "k_dw_bwd_weight<3,3>", "k_dw_bwd_weight<7,1> x 7"};
  const DwShape sh = {H, W, C, k, stride, pad, dil, (unsigned)features};
  const DwRoute r = (backward ? dw_bwd_route : dw_fwd_route)(sh, switches < 0 ? dw_switches() : (unsigned)switches);
  if (r.kern == DW_NONE || r.kern == DW_NARROW) return nullptr;
  static thread_local char buf[128];
  const char* fin = r.separate_finalize ? (backward ? "lhn_bn_bwd_finalize2 + " : "lhn_bn_finalize + ") : "";
  if (r.kern >= DWB_GATHER1) {
    const bool d = !(features & LHN_DW_F_NO_DX), wg = !(features & LHN_DW_F_NO_WEIGHT);
    snprintf(buf, sizeof(buf), "%s%s%s%s", fin, d ? gdata[r.kern - DWB_GATHER1] : "", d && wg ? " + " : "", wg ? gweight[r.kern - DWB_GATHER1] : "");
  } else {
    snprintf(buf, sizeof(buf), "%s%s%s", fin, name[r.kern], r.ps == 2 ? " ps=2" : "");
  }
  return buf;
}
