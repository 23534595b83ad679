// 1x1 (pointwise) convolution on fp32 MFMA, NHWC, with the producer's pending BatchNorm/activation
// applied on load and this layer's BatchNorm statistics accumulated in the epilogue.
//   Y[m][co] = sum_ci X[m][ci] * W[co][ci]        m = output pixel, X = consumed value of the input view
// Tile: 128 pixels x (32*NT) output channels per 256-thread block; wave w owns pixel rows [32w,32w+32).
// MFMA: v_mfma_f32_32x32x2_f32 (exact fp32 fma chain).  Operands come from LDS images with a +4 float
// row pad so that every ds_read_b128 is conflict-free (row stride = odd number of 16-B slots).
// K order inside an 8-wide chunk is permuted (lane half h supplies k = 8*kc + 4*h + j at step j); both
// operands use the same permutation, so only the fp32 summation order differs from a sequential loop.
#include <stdlib.h>
#include "lhn_common.h"

// Runtime geometry of ONE launch.  Wide or odd channel counts (hourglass C = 256, lite-hrnet 40/80/160/320) are run by the
// host as a grid of (<= 128 input channels) x (<= 128 output channels) launches over channel slices of the same buffers:
//   * the weight tensor keeps its own row stride (`wstride` floats), so a slice is just a pointer offset;
//   * `kvalid` input channels of the slice are real, the rest of the CIN-wide tile is zero (in A and in W);
//   * rows >= `wrows` of the slice have zero weights and zero bias (a 21-feature head stored in a 24-channel buffer);
//   * `yacc`: this launch ADDS to what the previous input slice stored (K split); bias and BatchNorm statistics belong to
//     the last slice, which sees the complete sum.
struct PwGeom {
  int wstride, kvalid, wrows, yacc, statC;
  int64_t nchw_bstride;      // floats between two images of the NCHW output
};

// stage a [rows][CIN] weight slice into LDS (row pad LDA): zero beyond wrows / kvalid; 16-byte loads when the slice allows
template <int CIN>
__device__ __forceinline__ void pw_stage_w(float* Ws, int LDA, const float* __restrict__ w, int rows_pad, const PwGeom& g) {
  constexpr int C4 = CIN / 4;
  const bool vec = (g.wstride % 4 == 0) && (g.kvalid % 4 == 0) && ((reinterpret_cast<uintptr_t>(w) & 15) == 0);
  for (int i = threadIdx.x; i < rows_pad * C4; i += 256) {
    const int co = i / C4, k4 = i % C4;
    f4 v = (f4){0.f, 0.f, 0.f, 0.f};
    if (co < g.wrows) {
      const float* r = w + (int64_t)co * g.wstride + k4 * 4;
      if (vec) {
        if (4 * k4 < g.kvalid) v = *reinterpret_cast<const f4*>(r);
      } else {
        if (4 * k4 + 0 < g.kvalid) v.x = r[0];
        if (4 * k4 + 1 < g.kvalid) v.y = r[1];
        if (4 * k4 + 2 < g.kvalid) v.z = r[2];
        if (4 * k4 + 3 < g.kvalid) v.w = r[3];
      }
    }
    *reinterpret_cast<f4*>(Ws + co * LDA + k4 * 4) = v;
  }
}

// Extra input sources: the consumed input is  sum_s coef[s] * value_s  (value = gate * act(BN(raw)) of source s; source 0 is
// `x`).  This is how the residual sums of MSRB (litehourglass.py:41-49: out + ca(cat), then out + x) reach the 1x1 without
// ever being written to HBM: summed on load.  All sources share x's geometry and channel range width.
struct PwExtra {
  lhn_view v[2];
  float coef[3];
  int n;             // number of EXTRA sources in v (0..2)
  float* sum_out;    // the summed input is ALSO written here (NULL: not): training needs it once, for the weight gradient
  int so_cstride, so_coff;
};

template <int CIN, int NT, int NS = 1>
__global__ void __launch_bounds__(256, NS > 1 ? 1 : ((CIN == 64 && NT == 2) || (CIN == 32 && NT == 4) ? 3 : (CIN == 64 && NT == 4) ? 2 : 1)) k_pw_fwd(lhn_view x, const float* __restrict__ w, const float* __restrict__ bias,
                                                lhn_view y, double* __restrict__ stats, int stride,
                                                float* __restrict__ y_nchw, int cout, int M, int ntiles, lhn_bnfin fin,
                                                PwGeom geo, PwExtra ex) {
  constexpr int LDA = CIN + 4;
  constexpr int PF = CIN / 8;   // float4 loads per thread per 128-pixel tile
  constexpr int C4 = CIN / 4;   // float4 per pixel row
  constexpr int RP = 256 / C4;  // rows covered per pass
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ws = smem;                    // [32*NT][LDA]
  float* As = smem + 32 * NT * LDA;    // [128][LDA]
  float* red = As;                     // [4][32*NT][2]: aliases the A tile after the last tile's trailing barrier
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: wave-uniform predicates become scalar branches)
  const int l31 = lane & 31, lh = lane >> 5;

  const int c4 = tid % C4, row0 = tid / C4;
  const bool kok = 4 * c4 < x.C;                     // channel groups beyond the view are zero columns of the tile
  const int cabs = x.coff + (kok ? 4 * c4 : 0);
  const int kleft = geo.kvalid - 4 * c4;             // real input channels from this thread's group on (>= 4: all four)
  const Xf4 xf = lhn_load_xf(x, cabs);
  const int HoWo = y.H * y.W;
  // extra sources (NS > 1): own buffer, table, gate, channel offset
  int ecabs[NS > 1 ? NS - 1 : 1];
  Xf4 exf[NS > 1 ? NS - 1 : 1];
  f4 epre[NS > 1 ? NS - 1 : 1][PF];
  if (NS > 1) {
#pragma unroll
    for (int e = 0; e < NS - 1; ++e)
      if (e < ex.n) {
        ecabs[e] = ex.v[e].coff + (kok ? 4 * c4 : 0);
        exf[e] = lhn_load_xf(ex.v[e], ecabs[e]);
      }
  }
  pw_stage_w<CIN>(Ws, LDA, w, 32 * NT, geo);

  f4 pre[PF];
  auto in_pix = [&](int m) __attribute__((always_inline)) -> int64_t {
    if (stride == 1) return m;
    const int n = m / HoWo, r = m - n * HoWo;
    const int ho = r / y.W, wo = r - ho * y.W;
    return ((int64_t)n * x.H + ho * stride) * x.W + wo * stride;
  };
  auto issue = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int m = tile * 128 + row0 + p * RP;
      pre[p] = (f4){0.f, 0.f, 0.f, 0.f};
      if (m < M && kok) pre[p] = *reinterpret_cast<const f4*>(x.data + in_pix(m) * x.cstride + cabs);
      if (NS > 1) {
#pragma unroll
        for (int e = 0; e < NS - 1; ++e)
          if (e < ex.n && m < M && kok)
            epre[e][p] = *reinterpret_cast<const f4*>(ex.v[e].data + (int64_t)m * ex.v[e].cstride + ecabs[e]);
      }
    }
  };
  auto commit = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int row = row0 + p * RP, m = tile * 128 + row;
      f4 v = (f4){0.f, 0.f, 0.f, 0.f};
      if (m < M && kok) {
        v = lhn_apply_xf(pre[p], xf);
        if (x.gate) v *= *reinterpret_cast<const f4*>(x.gate + (int64_t)(m / HoWo) * x.cstride + cabs);
        if (NS > 1) {
          v *= ex.coef[0];
#pragma unroll
          for (int e = 0; e < NS - 1; ++e)
            if (e < ex.n) {
              f4 u = lhn_apply_xf(epre[e][p], exf[e]);
              if (ex.v[e].gate) u *= *reinterpret_cast<const f4*>(ex.v[e].gate + (int64_t)(m / HoWo) * ex.v[e].cstride + ecabs[e]);
              v += u * ex.coef[e + 1];
            }
        }
        if (kleft < 4) {      // pad channels of a view wider than the weight (w_cols): zero weights do not cancel a NaN / inf
          if (kleft < 1) v.x = 0.f;
          if (kleft < 2) v.y = 0.f;
          if (kleft < 3) v.z = 0.f;
          v.w = 0.f;
        }
        if (NS > 1 && ex.sum_out) *reinterpret_cast<f4*>(ex.sum_out + (int64_t)m * ex.so_cstride + ex.so_coff + 4 * c4) = v;
      }
      *reinterpret_cast<f4*>(As + row * LDA + 4 * c4) = v;
    }
  };

  // BatchNorm statistics: shifted fp32 partial sums over ONE tile (16 values per lane), un-shifted into double per tile
  // (TileStat) -- a running fp32 sum of squares loses the variance when |mean| >> sigma (E[x^2] - E[x]^2 cancels)
  double ssum[NT], ssq[NT];
  float bv[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    ssum[nt] = ssq[nt] = 0.0;
    const int ch = nt * 32 + l31;
    bv[nt] = (bias && ch < geo.wrows) ? bias[ch] : 0.f;
  }

  int tile = blockIdx.x;
  if (tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    commit(tile);
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles) issue(next);

    f16v acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    const float* arow = As + (wave * 32 + l31) * LDA + 4 * lh;
    const float* brow = Ws + l31 * LDA + 4 * lh;
#pragma unroll 4
    for (int kc = 0; kc < CIN / 8; ++kc) {
      const f4 a = *reinterpret_cast<const f4*>(arow + kc * 8);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const f4 b = *reinterpret_cast<const f4*>(brow + nt * 32 * LDA + kc * 8);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[nt], 0, 0, 0);
      }
    }

    // epilogue: C/D layout col = lane&31 (channel), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (pixel)
    const int mbase = tile * 128 + wave * 32 + 4 * lh;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int ch = nt * 32 + l31;
      if (ch >= cout) continue;
      if (y_nchw) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int m0 = mbase + 8 * g;
          if (m0 < M) {  // HoWo % 4 == 0 is checked on the host: 4 consecutive pixels share an image
            const int n = m0 / HoWo, p = m0 - n * HoWo;
            f4 o = (f4){acc[nt][4 * g] + bv[nt], acc[nt][4 * g + 1] + bv[nt], acc[nt][4 * g + 2] + bv[nt],
                        acc[nt][4 * g + 3] + bv[nt]};
            f4* dst = reinterpret_cast<f4*>(y_nchw + (int64_t)n * geo.nchw_bstride + (int64_t)ch * HoWo + p);
            if (geo.yacc) o += *dst;
            *dst = o;
          }
        }
      } else {
        TileStat ts;
        ts.reset();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mbase + (r & 3) + 8 * (r >> 2);
          if (m < M) {
            float* dst = y.data + (int64_t)m * y.cstride + y.coff + ch;
            float v = acc[nt][r] + bv[nt];
            if (geo.yacc) v += *dst;
            *dst = v;
            ts.add(v);
          }
        }
        ts.flush(ssum[nt], ssq[nt]);
      }
    }
    __syncthreads();
  }

  if (stats) {
    double* redd = reinterpret_cast<double*>(red);       // [4][32*NT][2] doubles: 8 KB at NT = 4, inside the A tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const double s = ssum[nt] + __shfl_xor(ssum[nt], 32, 64);
      const double q = ssq[nt] + __shfl_xor(ssq[nt], 32, 64);
      if (lh == 0) {
        redd[(wave * 32 * NT + nt * 32 + l31) * 2 + 0] = s;
        redd[(wave * 32 * NT + nt * 32 + l31) * 2 + 1] = q;
      }
    }
    __syncthreads();
    if (tid < 32 * NT && tid < cout) {
      double s = 0, q = 0;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) {
        s += redd[(wv * 32 * NT + tid) * 2 + 0];
        q += redd[(wv * 32 * NT + tid) * 2 + 1];
      }
      double* st = stats + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * geo.statC;
      atomicAdd(st + tid, s);
      atomicAdd(st + geo.statC + tid, q);
    }
    if (fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block_par(fin, stats, redd);
  }
}

template <int CIN, int NT, int NS = 1>
static int launch_pw_fwd(const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats,
                         int stride, float* y_nchw, int cout, const lhn_bnfin* fin, const PwGeom& geo, hipStream_t s,
                         const PwExtra* exp = nullptr) {
  PwExtra ex;
  if (exp) ex = *exp; else { ex.n = 0; ex.sum_out = nullptr; }
  lhn_bnfin f;
  if (fin && stats) f = *fin; else f.counter = nullptr;
  const int M = y->N * y->H * y->W;
  const int ntiles = (M + 127) / 128;
  const size_t lds = (size_t)((32 * NT + 128) * (CIN + 4)) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_pw_fwd<CIN, NT, NS>, lds, 4, &per_cu)) {
    lhn_set_error("lhn_conv_pw_fwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  int grid = lhn_num_cus() * per_cu;
  if (grid > ntiles) grid = ntiles;
  hipLaunchKernelGGL((k_pw_fwd<CIN, NT, NS>), dim3(grid), dim3(256), lds, s, *x, w, bias, *y, stats, stride, y_nchw, cout, M,
                     ntiles, f, geo, ex);
  return 0;
}

// =====================================================================================================
// Forward, weights in REGISTERS (the fast path: stride 1, NHWC output, one input slice, Cout <= 128).
// A wave owns ONE 32-feature tile of W for the whole launch: its MFMA B fragments (CIN/2 VGPRs: lane = feature, lane half
// = k parity group) are loaded once from global memory.  LDS then only holds the pixel tile (double buffered, BM = 32..128
// pixels), 17..37 KB per block instead of 70..135 KB, so 2-3 blocks share a CU and one block's loads / LDS commit / stores
// run under another block's MFMA phase (the LDS-resident-W kernel above sits at ONE block per CU for 128 -> 128 and adds its
// phases up: 126 us against a 55 us MFMA bound).  Waves: NCOT feature tiles x (4 / NCOT) pixel sub-tiles of 32.
// Statistics need no cross-wave reduction: each wave owns its features.
// FIN: x is the output of a convolution + BatchNorm of CIN channels whose statistics are complete and whose table is not written yet
// (lhn_bnfinsrc): every workgroup folds the 32 replicas while its first tile's loads are in flight (the statistics' own loads go
// out in front of them), in the two pixel buffers, which nobody has
// committed to yet (CIN * 512 B of pairs from the front, the 3 * CIN table entries at the very end, in the second buffer, which
// the first commit does not reach), and workgroup 0 also stores what lhn_bn_finalize leaves in memory.  A template flag: the
// instances that do not fold keep their registers.
template <int CIN, int NCOT, int NS, bool FIN = false>
__global__ void __launch_bounds__(256, (NS > 1 || CIN >= 128) ? 2 : 3)
k_pw_fwd_wr(lhn_view x, const float* __restrict__ w, const float* __restrict__ bias, lhn_view y, double* __restrict__ stats,
            int cout, int M, int ntiles, PwExtra ex, int wstride, int yacc, int statC, int wt, lhn_bnfin fin, lhn_bnfinsrc fs) {
  constexpr int LDA = CIN + 4, PXW = 4 / NCOT, BM = 32 * PXW;
  constexpr int C4 = CIN / 4, RP = 256 / C4, PF = BM / RP;      // float4 loads per thread, tile and source
  static_assert(PF >= 1, "tile too small for the loader");
  extern __shared__ __attribute__((aligned(16))) float smem[];   // [2][BM][LDA]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int cot = wave % NCOT, pxs = wave / NCOT;
  const int co = cot * 32 + l31;
  // ---- B fragments: wreg[kc*4 + j] = W[co][8*kc + 4*lh + j]  (same K permutation as the A reads below)
  float wreg[CIN / 2];
#pragma unroll
  for (int kc = 0; kc < CIN / 8; ++kc) {
    f4 v = (f4){0.f, 0.f, 0.f, 0.f};
    if (co < cout) {
      if (!wt) v = *reinterpret_cast<const f4*>(w + (int64_t)co * wstride + kc * 8 + 4 * lh);      // wstride: row of the WHOLE weight
      else {      // transposed use (data gradient: out[ci] = sum_co dy[co] * W[co][ci]): feature `co` of this launch is a COLUMN of W
        const float* wc = w + (int64_t)(kc * 8 + 4 * lh) * wstride + co;
        v = (f4){wc[0], wc[wstride], wc[2 * (int64_t)wstride], wc[3 * (int64_t)wstride]};
      }
    }
    wreg[kc * 4 + 0] = v.x; wreg[kc * 4 + 1] = v.y; wreg[kc * 4 + 2] = v.z; wreg[kc * 4 + 3] = v.w;
  }
  const float bv = (bias && co < cout) ? bias[co] : 0.f;
  // ---- loader geometry
  const int c4 = tid % C4, row0 = tid / C4;
  const int cabs = x.coff + 4 * c4;
  const int HoWo = y.H * y.W;
  int ecabs[NS > 1 ? NS - 1 : 1];
  if (NS > 1) {
#pragma unroll
    for (int e = 0; e < NS - 1; ++e)
      if (e < ex.n) ecabs[e] = ex.v[e].coff + 4 * c4;
  }
  f4 pre[PF], epre[NS > 1 ? NS - 1 : 1][PF];
  Xf4 xf, exf[NS > 1 ? NS - 1 : 1];          // filled after the first tile's loads have been issued (see below)
  // gates: one sample per tile whenever H*W is a multiple of the tile (every map of the models here but 8x8 at BM = 128), so the
  // gate of a tile is ONE float4 per thread, fetched with the tile's pixels a tile ahead (the general commit below loads it per
  // row and waits for it: a vmcnt(0) in the middle of the loop that also drained the prefetch)
  const bool uni = HoWo % BM == 0;
  const f4 one4 = (f4){1.f, 1.f, 1.f, 1.f};
  f4 gpre = one4, egpre[NS > 1 ? NS - 1 : 1];
  auto issue = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int m = min(tile * BM + row0 + p * RP, M - 1);      // clamped: rows >= M are zeroed at commit
      pre[p] = *reinterpret_cast<const f4*>(x.data + (int64_t)m * x.cstride + cabs);
      if (NS > 1) {
#pragma unroll
        for (int e = 0; e < NS - 1; ++e)
          if (e < ex.n) epre[e][p] = *reinterpret_cast<const f4*>(ex.v[e].data + (int64_t)m * ex.v[e].cstride + ecabs[e]);
      }
    }
    if (uni) {
      const int n = min(tile * BM, M - 1) / HoWo;
      gpre = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + cabs) : one4;
      if (NS > 1) {
#pragma unroll
        for (int e = 0; e < NS - 1; ++e)
          if (e < ex.n) egpre[e] = ex.v[e].gate ? *reinterpret_cast<const f4*>(ex.v[e].gate + (int64_t)n * ex.v[e].cstride + ecabs[e]) : one4;
      }
    }
  };
  auto commit = [&](int tile, float* As) __attribute__((always_inline)) {
    // one straight-line form: rows >= M were loaded from a clamped (valid) address and are zeroed by a select, not a branch
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int row = row0 + p * RP, m = tile * BM + row;
      const bool ok = m < M;
      f4 g = gpre;
      if (!uni) {      // (a tile that spans samples: the gate per row)
        const int n = min(m, M - 1) / HoWo;
        g = x.gate ? *reinterpret_cast<const f4*>(x.gate + (int64_t)n * x.cstride + cabs) : one4;
      }
      f4 v = lhn_apply_xf(pre[p], xf) * g;
      if (NS > 1) {
        v *= ex.coef[0];
#pragma unroll
        for (int e = 0; e < NS - 1; ++e)
          if (e < ex.n) {
            f4 ge = egpre[e];
            if (!uni) {
              const int n = min(m, M - 1) / HoWo;
              ge = ex.v[e].gate ? *reinterpret_cast<const f4*>(ex.v[e].gate + (int64_t)n * ex.v[e].cstride + ecabs[e]) : one4;
            }
            v += lhn_apply_xf(epre[e][p], exf[e]) * ge * ex.coef[e + 1];
          }
        if (ex.sum_out && ok) *reinterpret_cast<f4*>(ex.sum_out + (int64_t)m * ex.so_cstride + ex.so_coff + 4 * c4) = v;
      }
      *reinterpret_cast<f4*>(As + row * LDA + 4 * c4) = ok ? v : (f4){0.f, 0.f, 0.f, 0.f};
    }
  };

  double ssum = 0.0, ssq = 0.0;       // fp32 partials per tile, promoted per tile (see k_pw_fwd)
  int tile = blockIdx.x, buf = 0;
  double fa[FIN ? CIN / 8 : 1], fb[FIN ? CIN / 8 : 1];      // FIN: this thread's share of the statistics, loaded in front of the tile
  LhnFinPre fpre;
  if constexpr (FIN) {
    fpre = lhn_bn_fin_pre(fs, 0, CIN, blockIdx.x == 0);
    lhn_bn_fin_load<CIN / 8>(fs.stats, CIN, 0, CIN, fa, fb);
  }
  if (tile < ntiles) issue(tile);     // the first tile's loads are in flight while pending BatchNorms are finalized
  if constexpr (FIN) {
    static_assert(NS == 1 && CIN % 8 == 0 && LHN_STAT_REPLICAS * CIN * 16 <= (2 * BM * LDA - 3 * CIN) * 4 && 3 * CIN <= BM * LDA &&
                      (2 * BM * LDA - 3 * CIN) % 4 == 0,
                  "the pixel buffers hold the replica pairs in front of the table entries, which sit in the second one");
    double* rawd = reinterpret_cast<double*>(smem);
    float* tab = smem + 2 * BM * LDA - 3 * CIN;
    const bool lead = blockIdx.x == 0;
    lhn_bn_fin_put<CIN / 8>(fa, fb, CIN, rawd);
    __syncthreads();
    if (tid < CIN) {
      constexpr int GC = LHN_FIN_THREADS / CIN > LHN_STAT_REPLICAS ? LHN_STAT_REPLICAS : LHN_FIN_THREADS / CIN;      // lhn_fin_groups(CIN)
      double s1, s2;
      lhn_bn_fin_sum<GC>(rawd, CIN, tid, GC, s1, s2);
      lhn_bn_fin_channel(fs, fpre, s1, s2, 0, tid, lead, tab, CIN);
    }
    __syncthreads();
    xf = lhn_bn_fin_xf(tab, CIN, 4 * c4);
  } else {
    xf = lhn_load_xf(x, cabs);
  }
  if (NS > 1) {
#pragma unroll
    for (int e = 0; e < NS - 1; ++e)
      if (e < ex.n) {
        exf[e] = lhn_load_xf(ex.v[e], ecabs[e]);
      }
  }
  if (tile < ntiles) {
    commit(tile, smem);
    if (tile + (int)gridDim.x < ntiles) issue(tile + gridDim.x);
  }
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x, buf ^= 1) {
    const float* As = smem + buf * BM * LDA;
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* arow = As + (pxs * 32 + l31) * LDA + 4 * lh;
#pragma unroll
    for (int kc = 0; kc < CIN / 8; ++kc) {
      const f4 a = *reinterpret_cast<const f4*>(arow + kc * 8);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wreg[kc * 4 + 0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wreg[kc * 4 + 1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wreg[kc * 4 + 2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wreg[kc * 4 + 3], acc, 0, 0, 0);
    }
    // next tile: registers -> the other LDS buffer (nobody reads it during this iteration), then the loads of the tile after
    const int next = tile + gridDim.x;
    if (next < ntiles) {
      commit(next, smem + (buf ^ 1) * BM * LDA);
      if (next + (int)gridDim.x < ntiles) issue(next + gridDim.x);
    }
    // epilogue: C/D layout col = lane&31 (feature), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (pixel)
    if (co < cout) {
      const int mbase = tile * BM + pxs * 32 + 4 * lh;
      float* yo = y.data + y.coff + co;
      TileStat ts;
      ts.reset();
      if (CIN < 256 && tile * BM + BM <= M && !yacc) {      // (K = 256 holds 128 registers of W: the batched stores below would spill)
        // whole tile inside the tensor (every tile but possibly the last): 16 plain stores off one base pointer.  The general
        // form below costs ~20 instructions and two branches per stored element (64-bit address product, row predicate, the
        // accumulate switch, the first-value select of TileStat) -- more issue slots than the tile's 16 MFMAs
        float* yp = yo + (int64_t)mbase * y.cstride;
        const int cs = y.cstride;
        const float k0 = acc[0] + bv;
        float sd = 0.f, qd = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[r] + bv;
          yp[((r & 3) + 8 * (r >> 2)) * cs] = v;
          const float d = v - k0;
          sd += d;
          qd += d * d;
        }
        ts.k = k0; ts.s = sd; ts.q = qd; ts.n = 16;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mbase + (r & 3) + 8 * (r >> 2);
          if (m < M) {
            float v = acc[r] + bv;
            if (yacc) v += yo[(int64_t)m * y.cstride];       // second K slice of a wide input (LHN_PW_K256=0), or the data gradient of a
                                                             // 256-feature convolution accumulating into dx (lhn_pw_dgrad_wr): statistics see the sum
            yo[(int64_t)m * y.cstride] = v;
            ts.add(v);
          }
        }
      }
      ts.flush(ssum, ssq);
    }
    __syncthreads();
  }
  if (stats && co < cout) {
    const double s = ssum + __shfl_xor(ssum, 32, 64), q = ssq + __shfl_xor(ssq, 32, 64);
    if (lh == 0) {
      double* st = stats + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * statC;      // statC: channels of the whole BatchNorm
      atomicAdd(st + co, s);
      atomicAdd(st + statC + co, q);
    }
  }
  // fused BatchNorm finalize (single-launch convolutions only, see pw_fwd_slice): the pixel tiles in LDS are dead by now
  if (stats && fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block_par(fin, stats, reinterpret_cast<double*>(smem));
}

template <int CIN, int NCOT, int NS, bool FIN = false>
static int launch_pw_fwd_wr(const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats, int cout,
                            hipStream_t s, const PwExtra* exp, const PwGeom& geo, int wt = 0, const lhn_bnfin* finp = nullptr,
                            const lhn_bnfinsrc* fsp = nullptr) {
  PwExtra ex;
  if (exp) ex = *exp; else { ex.n = 0; ex.sum_out = nullptr; }
  constexpr int BM = 32 * (4 / NCOT);
  const int M = y->N * y->H * y->W, ntiles = (M + BM - 1) / BM;
  const size_t lds = (size_t)2 * BM * (CIN + 4) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_pw_fwd_wr<CIN, NCOT, NS, FIN>, lds, 4, &per_cu)) {
    lhn_set_error("lhn_conv_pw_fwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  int grid = lhn_num_cus() * per_cu;      // (2 / 4 / 8 / 16 blocks per CU measured in round 3: forward 2.71 / 2.69 / 2.74 / 2.83 ms)
  if (grid > ntiles) grid = ntiles;
  lhn_bnfin fin;
  if (finp) fin = *finp; else fin.counter = nullptr;
  lhn_bnfinsrc fs;
  if (FIN && fsp) fs = *fsp; else memset(&fs, 0, sizeof(fs));
  hipLaunchKernelGGL((k_pw_fwd_wr<CIN, NCOT, NS, FIN>), dim3(grid), dim3(256), lds, s, *x, w, bias, *y, stats, cout, M, ntiles, ex, geo.wstride,
                     geo.yacc, geo.statC, wt, fin, fs);
  return 0;
}

// =====================================================================================================
// Backward: fused dgrad + wgrad.  Per 64-pixel tile the block stages
//     dYs[m][co] = dy  (formed on the fly from dz, the saved raw output y and the BN-backward coefficients)
//     Xs [m][ci] = consumed input value (raw input + the producer's pending transform / gate)
// and issues   dX[m][ci] = sum_co dYs[m][co] * W[co][ci]   (K = Cout)   -> global, store or accumulate
//              dW[co][ci] += sum_m dYs[m][co] * Xs[m][ci]  (K = 64)     -> registers across tiles, one
//                                                                           fp32 atomic add per block at the end
// NCHW = the head's gradient arrives as a plain NCHW tensor (dy_nchw); a template flag so that the NHWC instances do not
// carry its prefetch registers (they cost k_pw_bwd<64,2> 44 -> 56 us when the switch was a runtime one)
#ifndef LHN_PWB_BNS_OCC
#define LHN_PWB_BNS_OCC 3      // (2 = no spills: B step 8.45 vs 8.41 ms -- the 9 spilled registers cost less than the third workgroup gives)
#endif
template <int CIN, int NTO, bool NCHW, bool BNS = false>
__global__ void __launch_bounds__(256, (CIN == 32 && NTO == 1 && !NCHW) ? 4 : (CIN <= 64 && NTO <= 2 && !NCHW) ? (BNS ? LHN_PWB_BNS_OCC : 3) : 1) k_pw_bwd(lhn_view x, const float* __restrict__ w, lhn_view y, lhn_gradview gy,
                                                float* __restrict__ dx, int dx_acc, float* __restrict__ dw,
                                                float* __restrict__ dbias, int stride, const float* __restrict__ dy_nchw,
                                                int cout, int M, int ntiles, int nrep, int64_t rep_stride, PwGeom geo, lhn_bnsum bs) {
  constexpr int NTI = CIN / 32;
  constexpr int COP = 32 * NTO;
  constexpr int LDW = CIN + 4, LDY = COP + 4, LDX = CIN + 4;
  // MFMA work split: dX has 2*NTI tiles of 16*NTO MFMAs, dW has T = NTO*NTI tiles of 32 MFMAs (equal totals).  With
  // CIN = 32 (NTI == 1) dX only occupies waves 0,1, so dW goes to waves 2,3; when there are fewer dW tiles than dW
  // waves the 64-pixel K range of a tile is split across waves (partial sums meet in the final atomic flush).
  constexpr int T = NTO * NTI;
  constexpr bool DW_HI = (NTI == 1);
  constexpr int DWW = DW_HI ? 2 : 4;                   // waves that compute dW
  constexpr int KS = T < DWW ? DWW / T : 1;            // K parts per dW tile
  constexpr int NDW = (T * KS + DWW - 1) / DWW;        // dW accumulators per wave
  constexpr int NDX = (NTI + 1) / 2;                   // dX ci-tiles per wave
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ws = smem;                 // [COP][LDW]
  float* dYs = Ws + COP * LDW;      // [64][LDY]
  float* Xs = dYs + 64 * LDY;       // [64][LDX]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int HoWo = y.H * y.W;

  pw_stage_w<CIN>(Ws, LDW, w, COP, geo);

  // loader geometry: X tile 64 x CIN/4 float4, dY tile 64 x COP/4 float4
  constexpr int XC4 = CIN / 4, XRP = 256 / XC4, XPF = 64 / XRP;
  constexpr int YC4 = COP / 4, YRP = 256 / YC4, YPF = 64 / YRP;
  const int xc4 = tid % XC4, xr0 = tid / XC4;
  const bool xok = 4 * xc4 < x.C;      // channel groups beyond the input slice are zero columns
  const int xabs = x.coff + (xok ? 4 * xc4 : 0);
  const int yc4 = tid % YC4, yr0 = tid / YC4, yabs = y.coff + 4 * yc4;
  const Xf4 xxf = lhn_load_xf(x, xabs);
  const bool ych_ok = 4 * yc4 < cout;  // cout is a multiple of 4 on the NHWC path
  Xf4 yxf;
  Gr4 ygr;
  if (!NCHW && ych_ok) {
    yxf = lhn_load_xf(y, yabs);
    ygr = lhn_load_coef(gy, y.cstride, yabs);
  }
  f4 bsum = (f4){0.f, 0.f, 0.f, 0.f};

  f16v accw[NDW];
#pragma unroll
  for (int t = 0; t < NDW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) accw[t][r] = 0.f;

  auto in_pix = [&](int m) __attribute__((always_inline)) -> int64_t {
    if (stride == 1) return m;
    const int n = m / HoWo, r = m - n * HoWo;
    const int ho = r / y.W, wo = r - ho * y.W;
    return ((int64_t)n * x.H + ho * stride) * x.W + wo * stride;
  };

  // global loads of a tile go to registers (issue) one iteration ahead of their transform + LDS store (commit), so the
  // next tile's HBM latency overlaps this tile's MFMA work
  f4 xraw[XPF], yraw[YPF], ydz[YPF];
  constexpr int NCHW_PF = NCHW ? 64 * COP / 256 : 1;   // NCHW head: dY elements per thread and tile, prefetched like the rest
  float ynch[NCHW_PF];
  auto issue = [&](int tile) __attribute__((always_inline)) {
    if constexpr (NCHW) {
#pragma unroll
      for (int k = 0; k < NCHW_PF; ++k) {
        const int i = tid + 256 * k, row = i & 63, co = i >> 6, m = min(tile * 64 + row, M - 1);
        const int n = m / HoWo, p = m - n * HoWo;
        ynch[k] = co < cout ? dy_nchw[(int64_t)n * geo.nchw_bstride + (int64_t)co * HoWo + p] : 0.f;
      }
    }
#pragma unroll
    for (int p = 0; p < XPF; ++p) {
      const int m = min(tile * 64 + xr0 + p * XRP, M - 1);      // clamped (branch-free); commit() zeroes rows >= M
      xraw[p] = *reinterpret_cast<const f4*>(x.data + in_pix(m) * x.cstride + xabs);
    }
    if (!NCHW && ych_ok) {
#pragma unroll
      for (int p = 0; p < YPF; ++p) {
        const int m = min(tile * 64 + yr0 + p * YRP, M - 1);
        yraw[p] = *reinterpret_cast<const f4*>(y.data + (int64_t)m * y.cstride + yabs);
        ydz[p] = *reinterpret_cast<const f4*>(gy.dz + (int64_t)m * y.cstride + yabs);
      }
    }
  };
  auto commit = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < XPF; ++p) {
      const int row = xr0 + p * XRP, m = tile * 64 + row;
      f4 v = (f4){0.f, 0.f, 0.f, 0.f};
      if (m < M && xok) {
        v = lhn_apply_xf(xraw[p], xxf);
        if (x.gate) v *= *reinterpret_cast<const f4*>(x.gate + (int64_t)(m / HoWo) * x.cstride + xabs);
      }
      *reinterpret_cast<f4*>(Xs + row * LDX + 4 * xc4) = v;
    }
    if constexpr (NCHW) {
#pragma unroll
      for (int k = 0; k < NCHW_PF; ++k) {
        const int i = tid + 256 * k, row = i & 63, co = i >> 6;
        dYs[row * LDY + co] = (tile * 64 + row < M) ? ynch[k] : 0.f;
      }
    } else {
#pragma unroll
      for (int p = 0; p < YPF; ++p) {
        const int row = yr0 + p * YRP, m = tile * 64 + row;
        f4 v = (f4){0.f, 0.f, 0.f, 0.f};
        if (m < M && ych_ok) {
          const int n = m / HoWo, r = m - n * HoWo;
          const int h = r / y.W, ww = r - h * y.W;
          const f4 du = lhn_grad_du(y, gy, yxf, yraw[p], ydz[p], n, h, ww, yabs);
          v = ygr.A * du + ygr.B * yraw[p] + ygr.Cc;
          bsum += v;
        }
        *reinterpret_cast<f4*>(dYs + row * LDY + 4 * yc4) = v;
      }
    }
  };

  // bs.sums (lhn_bnsum): this launch's dX is (part of) the gradient of the value of x, the output of a convolution + BatchNorm
  // -- the lane that holds dX[m][ci] re-reads the raw x[m][ci] (the tile was just staged: L2) and adds du = dX * act'(u) and
  // du * xhat to its channel's sums; stride 1, host-checked.  Channel of lane and dX tile t: ci = 32 * ((wave >> 1) + 2 t) + l31.
  // (BNS is a template flag: as a runtime one its 14 registers spilled k_pw_bwd<64,2>)
  constexpr int NB = BNS ? NDX : 1;
  float b_sc[NB], b_sh[NB], b_sl[NB], b_mean[NB], b_inv[NB], b_s[NB], b_q[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t) {
    b_s[t] = b_q[t] = 0.f;
    const int ci = 32 * ((wave >> 1) + 2 * t) + l31;
    const bool ok = BNS && bs.sums && ci < x.C;
    b_sc[t] = ok && x.table ? x.table[x.coff + ci] : 1.f;
    b_sh[t] = ok && x.table ? x.table[x.cstride + x.coff + ci] : 0.f;
    b_sl[t] = ok && x.table ? x.table[2 * x.cstride + x.coff + ci] : 1.f;
    b_mean[t] = ok ? bs.save[bs.coff + ci] : 0.f;
    b_inv[t] = ok ? bs.save[bs.C + bs.coff + ci] : 0.f;
  }
  int tile = blockIdx.x;
  if (tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    commit(tile);
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) issue(tile + gridDim.x);

    // ---- dW += dY^T X   (K = 64 pixels)
    const int dwave = DW_HI ? wave - 2 : wave;
    if constexpr (!DW_HI && KS == 1 && T % 4 == 0 && 4 % NTI == 0) {
      // every wave owns whole dW tiles (tile wave + 4 t: row wave / NTI + (4 / NTI) t, column wave % NTI): no predicate around
      // the MFMAs -- with `if (tl < T)` here the compiler wrapped each one in exec-mask branches and lgkmcnt(0) waits (k_conv_kxk.hip)
      const float* ap = dYs + lh * LDY + l31 + 32 * (wave / NTI);
      const float* bp = Xs + lh * LDX + l31 + 32 * (wave % NTI);
#pragma unroll 4
      for (int ks = 0; ks < 32; ++ks) {
        const float b = bp[(2 * ks) * LDX];
        float a[NDW];
#pragma unroll
        for (int t = 0; t < NDW; ++t) a[t] = ap[(2 * ks) * LDY + 32 * (4 / NTI) * t];
#pragma unroll
        for (int t = 0; t < NDW; ++t) accw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b, accw[t], 0, 0, 0);
      }
    } else if (dwave >= 0) {
      const int kpart = KS > 1 ? dwave % KS : 0;
#pragma unroll 4
      for (int ks = kpart * (32 / KS); ks < (kpart + 1) * (32 / KS); ++ks) {
        const float* dyr = dYs + (2 * ks + lh) * LDY + l31;
        const float* xr = Xs + (2 * ks + lh) * LDX + l31;
#pragma unroll
        for (int t = 0; t < NDW; ++t) {
          const int tl = (dwave + DWW * t) / KS;
          if (tl < T) {
            const int it = tl / NTI, jt = tl % NTI;
            accw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(dyr[32 * it], xr[32 * jt], accw[t], 0, 0, 0);
          }
        }
      }
    }
    // ---- dX = dY W   (K = Cout)
    if (dx) {
      const int mt = wave & 1;
      f16v accx[NDX];
#pragma unroll
      for (int t = 0; t < NDX; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) accx[t][r] = 0.f;
      const float* arow = dYs + (mt * 32 + l31) * LDY + 4 * lh;
#pragma unroll 2
      for (int kc = 0; kc < COP / 8; ++kc) {
        const f4 a = *reinterpret_cast<const f4*>(arow + kc * 8);
        const float* wr = Ws + (kc * 8 + 4 * lh) * LDW + l31;
#pragma unroll
        for (int t = 0; t < NDX; ++t) {
          const int jt = (wave >> 1) + 2 * t;
          if (NTI % 2 == 0 || jt < NTI) {        // (even NTI: always true, folded at compile time)
            accx[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wr[0 * LDW + 32 * jt], accx[t], 0, 0, 0);
            accx[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wr[1 * LDW + 32 * jt], accx[t], 0, 0, 0);
            accx[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wr[2 * LDW + 32 * jt], accx[t], 0, 0, 0);
            accx[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wr[3 * LDW + 32 * jt], accx[t], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < NDX; ++t) {
        const int jt = (wave >> 1) + 2 * t;
        if (jt < NTI) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = tile * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (m < M && 32 * jt + l31 < x.C) {
              float* o = dx + in_pix(m) * x.cstride + x.coff + 32 * jt + l31;
              if (BNS) {
                const float raw = x.data[(int64_t)m * x.cstride + x.coff + 32 * jt + l31];
                const float du = accx[t][r] * (raw * b_sc[t] + b_sh[t] > 0.f ? 1.f : b_sl[t]);
                b_s[t] += du;
                b_q[t] += du * ((raw - b_mean[t]) * b_inv[t]);
              }
              *o = dx_acc ? *o + accx[t][r] : accx[t][r];
            }
          }
        }
      }
    }
    __syncthreads();
  }

  if (BNS) {      // the two lane halves and the two waves (pixel halves) of a channel tile meet in LDS (Xs is free now)
    float* bred = Xs;                                   // [NTI][2 waves][2][32]
#pragma unroll
    for (int t = 0; t < NB; ++t) {
      const int jt = (wave >> 1) + 2 * t;
      const float ss = b_s[t] + __shfl_xor(b_s[t], 32, 64), qq = b_q[t] + __shfl_xor(b_q[t], 32, 64);
      if (jt < NTI && lh == 0) {
        bred[((jt * 2 + (wave & 1)) * 2 + 0) * 32 + l31] = ss;
        bred[((jt * 2 + (wave & 1)) * 2 + 1) * 32 + l31] = qq;
      }
    }
    __syncthreads();
    if (tid < NTI * 32 && tid < x.C) {
      const int jt = tid >> 5, c = tid & 31;
      double* st = bs.sums + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * bs.C + bs.coff + tid;
      atomicAdd(st, (double)bred[((jt * 2 + 0) * 2 + 0) * 32 + c] + (double)bred[((jt * 2 + 1) * 2 + 0) * 32 + c]);
      atomicAdd(st + bs.C, (double)bred[((jt * 2 + 0) * 2 + 1) * 32 + c] + (double)bred[((jt * 2 + 1) * 2 + 1) * 32 + c]);
    }
    __syncthreads();
  }
  // ---- flush dW (C/D layout: row = co within tile, col = lane&31 = ci within tile)
  dw += (size_t)(blockIdx.x % nrep) * rep_stride;
#pragma unroll
  for (int t = 0; t < NDW; ++t) {
    const int dwave = DW_HI ? wave - 2 : wave;
    const int tl = dwave >= 0 ? (dwave + DWW * t) / KS : T;
    if (tl < T) {
      const int it = tl / NTI, jt = tl % NTI;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = 32 * it + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (co < geo.wrows && 32 * jt + l31 < geo.kvalid) atomicAdd(dw + (int64_t)co * geo.wstride + 32 * jt + l31, accw[t][r]);
      }
    }
  }
  if (dbias) {
    if (NCHW) {
      // head: few channels; recompute per-channel sums is cheap -- done by a separate tiny pass on the host side
    } else {
      // column sums of dy: the threads that share a channel group meet in LDS in a FIXED order (dYs is free by now), then
      // one add per channel into this block's gradient replica -- a single writer per address, like dW
      f4* bred = reinterpret_cast<f4*>(dYs);            // [YRP][YC4] float4 <= 64 * LDY floats
      bred[yr0 * YC4 + yc4] = ych_ok ? bsum : (f4){0.f, 0.f, 0.f, 0.f};
      __syncthreads();
      if (tid < YC4 && 4 * tid < cout) {
        f4 t = (f4){0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < YRP; ++j) t += bred[j * YC4 + tid];
        float* db = dbias + (size_t)(blockIdx.x % nrep) * rep_stride + 4 * tid;
        if (4 * tid + 0 < geo.wrows) atomicAdd(db + 0, t.x);
        if (4 * tid + 1 < geo.wrows) atomicAdd(db + 1, t.y);
        if (4 * tid + 2 < geo.wrows) atomicAdd(db + 2, t.z);
        if (4 * tid + 3 < geo.wrows) atomicAdd(db + 3, t.w);
      }
    }
  }
}

// bias gradient of the NCHW head: db[co] = sum_{n,p} dy[n,co,p]
__global__ void __launch_bounds__(256) k_bias_grad_nchw(const float* __restrict__ dy, float* __restrict__ db, int N, int C,
                                                        int HW, int64_t bstride) {
  const int co = blockIdx.x;
  double s = 0;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const float* p = dy + (int64_t)n * bstride + (int64_t)co * HW;
    float a = 0.f;
    for (int i = threadIdx.x; i < HW; i += blockDim.x) a += p[i];
    s += a;
  }
  s = lhn_wave_sum_d(s);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(db + co, (float)(red[0] + red[1] + red[2] + red[3]));
}

template <int CIN, int NTO, bool NCHW, bool BNS = false>
static int launch_pw_bwd_t(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_acc,
                         float* dw, float* dbias, int stride, const float* dy_nchw, int cout, int nrep, int64_t rep_stride,
                         const PwGeom& geo, hipStream_t s, const lhn_bnsum& bs) {
  const int M = y->N * y->H * y->W;
  const int ntiles = (M + 63) / 64;
  constexpr int COP = 32 * NTO;
  const size_t lds = (size_t)(COP * (CIN + 4) + 64 * (COP + 4) + 64 * (CIN + 4)) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_pw_bwd<CIN, NTO, NCHW, BNS>, lds, 4, &per_cu)) {
    lhn_set_error("lhn_conv_pw_bwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  int grid = lhn_num_cus() * per_cu;
  if (grid > ntiles) grid = ntiles;
  // (one tile per workgroup on small maps is the fastest split: fewer, longer workgroups -- 2 / 4 / 8 tiles each -- took Lite-HRNet's
  // step from 36.9 to 40.1 / 47.4 / 55.3 ms; the weight-gradient atomics are not what these launches wait for)
  lhn_gradview g = *gy;
  hipLaunchKernelGGL((k_pw_bwd<CIN, NTO, NCHW, BNS>), dim3(grid), dim3(256), lds, s, *x, w, *y, g, dx, dx_acc, dw, dbias, stride, dy_nchw,
                     cout, M, ntiles, nrep, rep_stride, geo, bs);
  if (dbias && dy_nchw)
    hipLaunchKernelGGL(k_bias_grad_nchw, dim3(geo.wrows, lhn_deterministic_mode() ? 1 : (y->N < 16 ? y->N : 16)), dim3(256), 0, s, dy_nchw, dbias, y->N, cout,
                       y->H * y->W, geo.nchw_bstride);
  return 0;
}

// =====================================================================================================
// Backward of the WIDE 1x1 (Cin * Cout >= 64 * 128, both <= 128; stride 1, NHWC, full-width weight, no reader-side sums) with the
// weights AND the weight gradient in registers: what k_pw_fwd_wr did for the forward.  k_pw_bwd<128,4> keeps W in LDS (135 KB with
// the two pixel tiles: one workgroup per CU, its phases add up), which is why these shapes went to lhn_pw_bwd_split: three launches
// and seven tensor passes (dz, y -> dy | dy -> dx | dy, x -> dW).  Here one launch reads dz, y, x and writes dx and dy:
//   dX: a wave owns ONE 32-wide input-channel tile for the whole launch; its slice of W is the MFMA B operand (K = COUT: COUT / 2
//       VGPRs per lane, loaded once from global memory).  CIN = 128: four tiles, a wave does every 32-pixel sub-tile of the tile;
//       CIN = 64: two tiles, waves pair up over the halves as in k_pw_bwd.
//   dW: the NTO * NTI 32x32 tiles are split four ways (tile row wave / NTI + (4 / NTI) t, column wave % NTI) and stay in accumulators
//       for the whole launch; one atomic flush per workgroup into its gradient replica.  No per-tile predicate in the loop.
//   LDS holds only the staged pixel tiles dYs / Xs and the per-channel tables (the pending transforms of x and y and the
//       BatchNorm-backward coefficients: 36 registers per thread in k_pw_bwd, re-read here from LDS at each commit), 38..55 KB:
//       two workgroups per CU (the register file decides, not LDS), so one's loads, commit and stores run under the other's MFMAs.
// dy is ALSO stored over dz, as k_dy_inplace does on the split path: the callers of lhn_conv_pw_bwd3 see the same buffers whichever
// path ran (tests/test_pw_gpu.py pins dz = dy for these shapes) -- unless the caller declares dz dead (lhn_conv_pw_bwd6,
// LHN_PW_BWD_DZ_DEAD): the DYST = false instances of the same shapes keep dy in LDS and save the write pass (the plan executor's
// calls: 134 MB per launch on variant B's 64^2 maps at batch 64).  PX: pixels per tile (64, or 32 where 64 does not fit the registers).
// PF: what rides in the register prefetch one tile ahead, 0 = x, 1 = x and y, 2 = x, y and dz; the rest is fetched inside commit()
// four rows at a time, so that its registers are not live across the MFMA phase.
//
// The NARROW shapes (64 -> 64, 32 -> 32; k_pw_bwd's largest launches on the big maps) run here too, registers to spare:
//   DYST = false: dz is only read (the callers of the fused path rely on that), one write pass less per tile.
//   64 -> 64: as CIN = 64 above with one dW tile per wave.
//   32 -> 32: one channel tile on each side, PX = 128: wave v takes pixels [32 v, 32 v + 32) of the tile in dX AND in dW (its own
//       quarter of K for the whole launch, no predicate in the loop); the four partial 32x32 tiles meet in LDS in wave order at the
//       flush, then one add per element into the workgroup's replica.
//   BNS: reader-side BatchNorm sums (lhn_bnsum) with the meaning they have in k_pw_bwd: the lane that holds dX[m][ci] adds
//       du = dX * act'(u) and du * xhat to its channel's sums.  A wave keeps ONE channel tile, so the channel's constants are five
//       registers; raw x comes from an LDS copy of the staged tile (Xr, written at commit in these instances only) where k_pw_bwd
//       re-read it from global memory.  Rows beyond M are zero rows of dYs: their dX is exactly 0 and adds nothing.
// OCC: workgroups per CU the register budget is cut for (waves per SIMD of __launch_bounds__).
// PF = 3 (32 -> 32 only, launched for dx_acc != 0 only): the prior dx rides in the prefetch as well, one more tensor of the tile.  It is
//   loaded in issue() with x's loader geometry, parked by commit() in the LDS tile Pr and read in the C/D layout at the store,
//   dx = prior + dX: the same fp32 add of the same two values as the read-modify-write `dx += dX` of the other instances, so the bits
//   of dx are the same.  That read-modify-write's sixteen loads per lane are issued behind issue(next tile), and vmcnt counts in
//   order: waiting for them waits for the whole prefetch, which then no longer runs under the MFMA phase and the stores.
template <int CIN, int COUT, int PX, int PF, bool DYST, bool BNS, int OCC>
__global__ void __launch_bounds__(256, OCC) k_pw_bwd_wr(lhn_view x, const float* __restrict__ w, lhn_view y, lhn_gradview gy,
                                                        float* __restrict__ dx, int dx_acc, float* __restrict__ dw, float* __restrict__ dbias,
                                                        int M, int ntiles, int nrep, int64_t rep_stride, lhn_bnsum bs, lhn_bnbwdsrc fs) {
  constexpr int NTI = CIN / 32, NTO = COUT / 32, LDY = COUT + 4, LDX = CIN + 4;
  constexpr bool ONE = NTI == 1;                // 32 -> 32: the single dW tile is split over the waves by pixels, not by tiles
  constexpr int NDW = ONE ? 1 : NTO * NTI / 4;  // dW tiles per wave
  constexpr int KW = ONE ? 32 : PX;             // pixels of a tile that one wave sums into its dW tiles
  constexpr int NDX = (NTI == 4 && PX == 64) ? 2 : 1;      // 32-pixel sub-tiles of dX per wave
  constexpr int NWC = 4 / NTI;                  // waves that share an input-channel tile in dX (BNS: partial sums per channel)
  static_assert(ONE ? (NTO == 1 && PX == 128) : ((NTI == 2 || NTI == 4) && (NTO == 2 || NTO == 4) && (PX == 64 || (PX == 32 && NTI == 4))),
                "32 -> 32 at 128 pixels; 64 / 128 channels on either side at 64 (or 32) pixels");
  static_assert(!BNS || NDX == 1, "reader-side sums: one dX sub-tile per wave");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dYs = smem;                  // [PX][LDY]
  float* Xs = dYs + PX * LDY;         // [PX][LDX]
  float* xt = Xs + PX * LDX;          // [3][CIN]   scale | shift | slope of x
  float* yt = xt + 3 * CIN;           // [3][COUT]  the same of y
  float* cf = yt + 3 * COUT;          // [3][COUT]  A | B | C
  float* Xr = cf + 3 * COUT;          // [PX][CIN]  raw x of the staged tile (BNS only)
  float* Pr = Xr + (BNS ? PX * CIN : 0);      // [PX][CIN]  prior dx of the staged tile (PF = 3 only)
  constexpr bool ACCPF = PF == 3;
  static_assert(!ACCPF || (ONE && !DYST), "the prior dx in the prefetch: 32 -> 32");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int HoWo = y.H * y.W;
  float* dzw = const_cast<float*>(gy.dz);

  constexpr int XC4 = CIN / 4, XRP = 256 / XC4, XPF = PX / XRP;
  constexpr int YC4 = COUT / 4, YRP = 256 / YC4, YPF = PX / YRP;
  constexpr int ZCH = YPF < 4 ? YPF : 4;
  const int xc4 = tid % XC4, xr0 = tid / XC4, xabs = x.coff + 4 * xc4;
  const int yc4 = tid % YC4, yr0 = tid / YC4, yabs = y.coff + 4 * yc4;

  f4 xraw[XPF], yraw[YPF], ydz[YPF], praw[ACCPF ? XPF : 1];
  auto issue = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < XPF; ++p) {
      const int m = min(tile * PX + xr0 + p * XRP, M - 1);      // clamped (branch-free); commit() zeroes rows >= M
      xraw[p] = *reinterpret_cast<const f4*>(x.data + (int64_t)m * x.cstride + xabs);
      if (ACCPF) praw[p] = *reinterpret_cast<const f4*>(dx + (int64_t)m * x.cstride + xabs);      // (rows >= M: never stored)
    }
#pragma unroll
    for (int p = 0; p < YPF; ++p) {
      const int m = min(tile * PX + yr0 + p * YRP, M - 1);
      if (PF >= 1) yraw[p] = *reinterpret_cast<const f4*>(y.data + (int64_t)m * y.cstride + yabs);
      if (PF >= 2) ydz[p] = *reinterpret_cast<const f4*>(gy.dz + (int64_t)m * y.cstride + yabs);
    }
  };
  f4 bsum = (f4){0.f, 0.f, 0.f, 0.f};
  auto commit = [&](int tile) __attribute__((always_inline)) {
    Xf4 xxf;
    xxf.sc = *reinterpret_cast<const f4*>(xt + 4 * xc4);
    xxf.sh = *reinterpret_cast<const f4*>(xt + CIN + 4 * xc4);
    xxf.sl = *reinterpret_cast<const f4*>(xt + 2 * CIN + 4 * xc4);
#pragma unroll
    for (int p = 0; p < XPF; ++p) {
      const int row = xr0 + p * XRP, m = tile * PX + row;
      f4 v = (f4){0.f, 0.f, 0.f, 0.f};
      if (m < M) {
        v = lhn_apply_xf(xraw[p], xxf);
        if (!BNS && x.gate) v *= *reinterpret_cast<const f4*>(x.gate + (int64_t)(m / HoWo) * x.cstride + xabs);      // (sums: no gate, host-checked)
      }
      *reinterpret_cast<f4*>(Xs + row * LDX + 4 * xc4) = v;
      if (BNS) *reinterpret_cast<f4*>(Xr + row * CIN + 4 * xc4) = m < M ? xraw[p] : (f4){0.f, 0.f, 0.f, 0.f};
      if (ACCPF) *reinterpret_cast<f4*>(Pr + row * CIN + 4 * xc4) = praw[p];
    }
    Xf4 yxf;
    Gr4 ygr;
    yxf.sc = *reinterpret_cast<const f4*>(yt + 4 * yc4);
    yxf.sh = *reinterpret_cast<const f4*>(yt + COUT + 4 * yc4);
    yxf.sl = *reinterpret_cast<const f4*>(yt + 2 * COUT + 4 * yc4);
    ygr.A = *reinterpret_cast<const f4*>(cf + 4 * yc4);
    ygr.B = *reinterpret_cast<const f4*>(cf + COUT + 4 * yc4);
    ygr.Cc = *reinterpret_cast<const f4*>(cf + 2 * COUT + 4 * yc4);
#pragma unroll
    for (int p = 0; p < YPF; ++p) {
      if (PF < 2 && p % ZCH == 0) {      // what was not prefetched (its registers would be live across the MFMA phase): the next ZCH rows
#pragma unroll
        for (int q = p; q < p + ZCH; ++q) {
          const int mq = min(tile * PX + yr0 + q * YRP, M - 1);
          if (PF < 1) yraw[q] = *reinterpret_cast<const f4*>(y.data + (int64_t)mq * y.cstride + yabs);
          ydz[q] = *reinterpret_cast<const f4*>(gy.dz + (int64_t)mq * y.cstride + yabs);
        }
      }
      const int row = yr0 + p * YRP, m = tile * PX + row;
      f4 v = (f4){0.f, 0.f, 0.f, 0.f};
      if (m < M) {
        int n = 0, h = 0, ww = 0;
        if (y.gate || gy.dpool) {          // (pixel coordinates only where lhn_grad_du reads them)
          n = m / HoWo;
          const int r = m - n * HoWo;
          h = r / y.W;
          ww = r - h * y.W;
        }
        const f4 du = lhn_grad_du(y, gy, yxf, yraw[p], ydz[p], n, h, ww, yabs);
        v = ygr.A * du + ygr.B * yraw[p] + ygr.Cc;
        bsum += v;
        if (DYST) *reinterpret_cast<f4*>(dzw + (int64_t)m * y.cstride + yabs) = v;
      }
      *reinterpret_cast<f4*>(dYs + row * LDY + 4 * yc4) = v;
    }
  };

  int tile = blockIdx.x;
  if (tile < ntiles) issue(tile);     // the first tile's loads are in flight while the tables and W are fetched
  // BatchNorm-backward finalize of y in the prologue (lhn_bnbwdsrc): the replica fold's loads go out behind the tile's, its 1,024
  // group partials wait in dYs (16 KB; commit() writes it only after the barrier below) while the tables and W are fetched
  static_assert(PX * LDY * sizeof(float) >= 2 * LHN_FIN_THREADS * sizeof(double), "dYs holds the replica fold's partials");
  LhnBwdPre fpre;
  if (fs.sums) {
    fpre = lhn_bn_bwd_pre(fs, 0, COUT);
    lhn_bn_bwd_fold_part_ct<COUT>(fs.sums, fs.stat_channels, reinterpret_cast<double*>(dYs));
  }
  for (int i = tid; i < CIN; i += 256) {
    xt[i] = x.table ? x.table[x.coff + i] : 1.f;
    xt[CIN + i] = x.table ? x.table[x.cstride + x.coff + i] : 0.f;
    xt[2 * CIN + i] = x.table ? x.table[2 * x.cstride + x.coff + i] : 1.f;
  }
  for (int i = tid; i < COUT; i += 256) {
    yt[i] = y.table ? y.table[y.coff + i] : 1.f;
    yt[COUT + i] = y.table ? y.table[y.cstride + y.coff + i] : 0.f;
    yt[2 * COUT + i] = y.table ? y.table[2 * y.cstride + y.coff + i] : 1.f;
    if (fs.sums) continue;            // A | B | C come out of the fold below
    cf[i] = gy.coef ? gy.coef[y.coff + i] : 1.f;
    cf[COUT + i] = gy.coef ? gy.coef[y.cstride + y.coff + i] : 0.f;
    cf[2 * COUT + i] = gy.coef ? gy.coef[2 * y.cstride + y.coff + i] : 0.f;
  }
  // ---- B fragments of the data gradient: wreg[kc*4 + j] = W[8*kc + 4*lh + j][32*jt + l31]  (K permutation of the dYs reads below)
  const int jt = NTI == 4 ? wave : NTI == 2 ? wave >> 1 : 0;
  const int mt0 = NTI == 4 ? 0 : NTI == 2 ? (wave & 1) : wave;      // first 32-pixel sub-tile of the wave in dX
  float wreg[COUT / 2];
#pragma unroll
  for (int k = 0; k < COUT / 2; ++k) wreg[k] = dx ? w[(int64_t)((k >> 2) * 8 + 4 * lh + (k & 3)) * CIN + 32 * jt + l31] : 0.f;
  f16v accw[NDW];
#pragma unroll
  for (int t = 0; t < NDW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) accw[t][r] = 0.f;
  // reader-side sums: the constants of this lane's channel 32 jt + l31 and its two partial sums
  float b_sc = 1.f, b_sh = 0.f, b_sl = 1.f, b_mean = 0.f, b_inv = 0.f, b_s = 0.f, b_q = 0.f;
  if (BNS) {
    const int ci = 32 * jt + l31;
    if (x.table) {
      b_sc = x.table[x.coff + ci];
      b_sh = x.table[x.cstride + x.coff + ci];
      b_sl = x.table[2 * x.cstride + x.coff + ci];
    }
    b_mean = bs.save[bs.coff + ci];
    b_inv = bs.save[bs.C + bs.coff + ci];
  }
  // (the flush address of this thread's channel, formed once)
  double* const bst = BNS ? bs.sums + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * bs.C + bs.coff + (tid & (CIN - 1)) : nullptr;
  const int bsC = BNS ? bs.C : 0;
  if (fs.sums) {      // thread c: the groups in order, the coefficients into cf; workgroup 0 also leaves them (and dgamma, dbeta) in memory
    __syncthreads();
    if (tid < COUT)
      lhn_bn_bwd_coef_put(lhn_bn_bwd_coef(reinterpret_cast<const double*>(dYs), COUT, LHN_FIN_THREADS / COUT, tid, fpre.gamma, fpre.mean,
                                          fpre.inv, fs.count),
                          fs, const_cast<float*>(gy.coef), y.cstride, y.coff, tid, cf, COUT, tid, blockIdx.x == 0);
  }
  __syncthreads();

  for (; tile < ntiles; tile += gridDim.x) {
    commit(tile);
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) issue(tile + gridDim.x);
    // ---- dW += dY^T X   (K = KW pixels: the whole tile, or this wave's quarter of it)
    {
      const float* ap = dYs + ((ONE ? 32 * wave : 0) + lh) * LDY + l31 + (ONE ? 0 : 32 * (wave / NTI));
      const float* bp = Xs + ((ONE ? 32 * wave : 0) + lh) * LDX + l31 + (ONE ? 0 : 32 * (wave % NTI));
#pragma unroll 4
      for (int ks = 0; ks < KW / 2; ++ks) {
        const float b = bp[(2 * ks) * LDX];
        float a[NDW];
#pragma unroll
        for (int t = 0; t < NDW; ++t) a[t] = ap[(2 * ks) * LDY + 32 * (4 / NTI) * t];
#pragma unroll
        for (int t = 0; t < NDW; ++t) accw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b, accw[t], 0, 0, 0);
      }
    }
    // ---- dX = dY W   (K = COUT)
    if (dx) {
      f16v accx[NDX];
#pragma unroll
      for (int hh = 0; hh < NDX; ++hh)
#pragma unroll
        for (int r = 0; r < 16; ++r) accx[hh][r] = 0.f;
      const float* arow = dYs + (mt0 * 32 + l31) * LDY + 4 * lh;
#pragma unroll
      for (int kc = 0; kc < COUT / 8; ++kc) {
#pragma unroll
        for (int hh = 0; hh < NDX; ++hh) {
          const f4 a = *reinterpret_cast<const f4*>(arow + hh * 32 * LDY + kc * 8);
          accx[hh] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, wreg[kc * 4 + 0], accx[hh], 0, 0, 0);
          accx[hh] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, wreg[kc * 4 + 1], accx[hh], 0, 0, 0);
          accx[hh] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, wreg[kc * 4 + 2], accx[hh], 0, 0, 0);
          accx[hh] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, wreg[kc * 4 + 3], accx[hh], 0, 0, 0);
        }
      }
      // C/D layout: col = lane&31 (input channel), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (pixel)
      const int cs = x.cstride;
#pragma unroll
      for (int hh = 0; hh < NDX; ++hh) {
        const int mbase = tile * PX + (mt0 + hh) * 32 + 4 * lh;
        float* o = dx + (int64_t)mbase * cs + x.coff + 32 * jt + l31;
        if (BNS) {
          const float* xr = Xr + ((mt0 + hh) * 32 + 4 * lh) * CIN + 32 * jt + l31;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float raw = xr[((r & 3) + 8 * (r >> 2)) * CIN];
            const float du = accx[hh][r] * (raw * b_sc + b_sh > 0.f ? 1.f : b_sl);
            b_s += du;
            b_q += du * ((raw - b_mean) * b_inv);
          }
        }
        if constexpr (ACCPF) {            // the prior of this lane's sixteen elements from the LDS tile: no load behind issue(next)
          const float* pr = Pr + ((mt0 + hh) * 32 + 4 * lh) * CIN + 32 * jt + l31;
          if (tile * PX + PX <= M) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[((r & 3) + 8 * (r >> 2)) * cs] = pr[((r & 3) + 8 * (r >> 2)) * CIN] + accx[hh][r];
          } else {                        // the tail tile: rows predicated per lane
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int ro = (r & 3) + 8 * (r >> 2);
              if (mbase + ro < M) o[(int64_t)ro * cs] = pr[ro * CIN] + accx[hh][r];
            }
          }
        } else if (tile * PX + PX <= M) {        // whole tile inside the tensor: stores off one base pointer, no row predicate
          if (dx_acc) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[((r & 3) + 8 * (r >> 2)) * cs] += accx[hh][r];
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[((r & 3) + 8 * (r >> 2)) * cs] = accx[hh][r];
          }
        } else if constexpr (BNS) {      // the tail tile with row offsets per lane: as scalars, next to the sums' own, they spilled 22 SGPRs
          float* ot = dx + (int64_t)(tile * PX + (mt0 + hh) * 32) * cs + x.coff + 32 * jt + l31;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ro = (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (tile * PX + (mt0 + hh) * 32 + ro < M) ot[(int64_t)ro * cs] = dx_acc ? ot[(int64_t)ro * cs] + accx[hh][r] : accx[hh][r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ro = (r & 3) + 8 * (r >> 2);
            if (mbase + ro < M) o[ro * cs] = dx_acc ? o[ro * cs] + accx[hh][r] : accx[hh][r];
          }
        }
      }
    }
    __syncthreads();
  }

  if (BNS) {      // lane halves by shuffle, the NWC waves of a channel tile in LDS in wave order (Xs is free now), one add per channel
    float* bred = Xs;                                   // [NTI][NWC][2][32]
    const float ss = b_s + __shfl_xor(b_s, 32, 64), qq = b_q + __shfl_xor(b_q, 32, 64);
    if (lh == 0) {
      bred[((jt * NWC + mt0) * 2 + 0) * 32 + l31] = ss;
      bred[((jt * NWC + mt0) * 2 + 1) * 32 + l31] = qq;
    }
    __syncthreads();
    if (tid < CIN) {
      const int jc = tid >> 5, c = tid & 31;
      double ds = 0.0, dq = 0.0;
#pragma unroll
      for (int v = 0; v < NWC; ++v) {
        ds += (double)bred[((jc * NWC + v) * 2 + 0) * 32 + c];
        dq += (double)bred[((jc * NWC + v) * 2 + 1) * 32 + c];
      }
      atomicAdd(bst, ds);
      atomicAdd(bst + bsC, dq);
    }
  }
  // ---- flush dW (C/D layout: row = co within the tile, col = lane&31 = ci within the tile): one add per element and workgroup
  dw += (size_t)(blockIdx.x % nrep) * rep_stride;
  if constexpr (ONE) {      // the four pixel quarters of the one tile: summed in wave order (dYs is free: the loop ended at a barrier)
    float* wred = dYs;                                  // [4 waves][16][64 lanes] <= PX * LDY floats
#pragma unroll
    for (int r = 0; r < 16; ++r) wred[(wave * 16 + r) * 64 + lane] = accw[0][r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 4 * q + wave, co = (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float v = ((wred[r * 64 + lane] + wred[(16 + r) * 64 + lane]) + wred[(32 + r) * 64 + lane]) + wred[(48 + r) * 64 + lane];
      atomicAdd(dw + (int64_t)co * CIN + l31, v);
    }
    if (dbias) __syncthreads();      // (dbias stages in dYs as well)
  } else {
#pragma unroll
    for (int t = 0; t < NDW; ++t) {
      const int it = wave / NTI + (4 / NTI) * t, jw = wave % NTI;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = 32 * it + (r & 3) + 8 * (r >> 2) + 4 * lh;
        atomicAdd(dw + (int64_t)co * CIN + 32 * jw + l31, accw[t][r]);
      }
    }
  }
  if (dbias) {      // column sums of dy in a fixed order, one add per channel into the workgroup's replica (as k_pw_bwd; dYs is free)
    f4* bred = reinterpret_cast<f4*>(dYs);            // [YRP][YC4] float4
    bred[yr0 * YC4 + yc4] = bsum;
    __syncthreads();
    if (tid < YC4) {
      f4 t = (f4){0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < YRP; ++j) t += bred[j * YC4 + tid];
      float* db = dbias + (size_t)(blockIdx.x % nrep) * rep_stride + 4 * tid;
      atomicAdd(db + 0, t.x);
      atomicAdd(db + 1, t.y);
      atomicAdd(db + 2, t.z);
      atomicAdd(db + 3, t.w);
    }
  }
}

// Instances (compiler's resource report, two workgroups per CU = 256 registers per lane):
//   128 -> 128: PX = 32, x and y prefetched.  With 64-pixel tiles the budget of 64 (W) + 64 (dW) + 32 (dX) + staging does not close:
//               61..133 registers spill whichever tensors ride in the prefetch (the dX phase with two sub-tiles is the peak).
//   64 -> 128:  PX = 64, x and y prefetched (dz too: 1 spill).      128 -> 64: PX = 64, x, y and dz prefetched.
// Narrow instances (no dy store; plain and with reader-side sums):
//   64 -> 64:   PX = 64, x, y and dz prefetched, two workgroups per CU (a third costs spills).
//   32 -> 32:   PX = 128, x, y and dz prefetched.
//               An accumulating launch (dx_acc != 0; the stem's b1 -> b3, whose input also feeds the max pool) runs PF = 3, the
//               prior dx in the prefetch too (LDS + 16 KB), at two workgroups per CU also where the plain instance has three: its
//               16 more registers do not fit the budget of three.  lhn_conv_pw_route answers with the PF = 2 instance either way.
//   64 -> 64 keeps the read-modify-write: no plan of the project launches it accumulating, and with sums it has 6 registers left.
// LHN_PW_BWD_ACC_PREFETCH (default 1), read once.  0: an accumulating 32 -> 32 launch re-reads dx at its store, as before PF = 3.
static bool pw_bwd_acc_prefetch_on() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("LHN_PW_BWD_ACC_PREFETCH");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v != 0;
}
template <int CIN, int COUT, int PX, int PF, bool DYST = true, bool BNS = false, int OCC = 2>
static int launch_pw_bwd_wr(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_acc, float* dw,
                            float* dbias, int nrep, int64_t rep_stride, hipStream_t s, const lhn_bnsum& bs, const lhn_bnbwdsrc* fsp = nullptr,
                            int det_per_cu = 0) {
  if constexpr (CIN == 32 && COUT == 32 && PF == 2) {      // (deterministic mode: the grid of THIS instance, so that every sum keeps its order)
    if (dx && dx_acc && pw_bwd_acc_prefetch_on())
      return launch_pw_bwd_wr<CIN, COUT, PX, 3, DYST, BNS, 2>(x, w, y, gy, dx, dx_acc, dw, dbias, nrep, rep_stride, s, bs, fsp, OCC);
  }
  const int M = y->N * y->H * y->W, ntiles = (M + PX - 1) / PX;
  lhn_bnbwdsrc fs;
  if (fsp) fs = *fsp; else memset(&fs, 0, sizeof(fs));
  const size_t lds = (size_t)(PX * (COUT + 4) + PX * (CIN + 4) + 3 * CIN + 6 * COUT + (BNS ? PX * CIN : 0) + (PF == 3 ? PX * CIN : 0)) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_pw_bwd_wr<CIN, COUT, PX, PF, DYST, BNS, OCC>, lds, OCC, &per_cu)) {
    lhn_set_error("lhn_conv_pw_bwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  int grid = lhn_num_cus() * ((det_per_cu && lhn_deterministic_mode()) ? det_per_cu : per_cu);
  if (grid > ntiles) grid = ntiles;
  hipLaunchKernelGGL((k_pw_bwd_wr<CIN, COUT, PX, PF, DYST, BNS, OCC>), dim3(grid), dim3(256), lds, s, *x, w, *y, *gy, dx, dx_acc, dw, dbias,
                     M, ntiles, nrep, rep_stride, bs, fs);
  return 0;
}

// =====================================================================================================
// Route: which kernels a 1x1 call launches.  pw_fwd_route() and pw_bwd_route() are pure and the only place that knows the rules; the
// dispatchers below and lhn_conv_pw_route() (the host-only query, which the tests and profiles/pw_instances.md read) call them.
struct PwShape {
  int N, H, W, HoWo;             // of x; pixels of one output image
  int Cin, Cout, stride;
  int wcols, wrows;              // the weight tensor's real shape (<= Cin, <= Cout)
  unsigned f;                    // LHN_PW_F_*: what the call carries
};
enum PwPath {
  PW_NONE = 0,      // no instance
  PW_HEAD,          // the streaming head kernels (k_conv_head.hip)
  PW_SLICED,        // (<= 128 | 256) x (<= 128) channel slices on k_pw_fwd_wr / k_pw_fwd; backward: the fused k_pw_bwd
  PWB_WIDE,         // backward, one register-W launch: 128 -> 128, 64 -> 128, 128 -> 64
  PWB_NARROW,       // the same kernel's 64 -> 64 and 32 -> 32 instances
  PWB_SPLIT         // k_dy_inplace, dgrad, wgrad (lhn_pw_bwd_split)
};
struct PwRoute {
  PwPath path;
  int kstep;                     // sliced forward: input channels per launch, 128 or 256 (the whole K = 256 on the register-W kernel)
  int dgrad;                     // split: LHN_PW_DGRAD_*, the kernel every output slice's data gradient takes
  bool dyst, bns;                // wide / narrow: DYST and BNS of the k_pw_bwd_wr instance
  bool separate_finalize;        // forward: the sliced form's own lhn_bn_finalize launch behind; backward: lhn_bn_bwd_finalize2 in front
  bool gate_reduce_after;        // gate sums asked for and the kernel does not add them: the lhn_gate_bwd_reduce3 launch behind
  bool finalize_in_front;        // forward: a finalize source (lhn_bnfinsrc) that no kernel folds: the lhn_bn_finalize launch of x's BatchNorm
};
// One forward launch of the sliced path: k_pw_fwd_wr<ci, nt, ns> (wr; nt = NCOT) or k_pw_fwd<ci, nt, ns>.  ci = 0: no instance.
struct PwInst {
  int ci, nt, ns;
  bool wr;
  bool fin;                      // the register-W instance that folds a finalize source in its prologue (FIN)
};

// LHN_PW_SW_*, read from the environment once.  LHN_PW_LDSW=1: no register-W kernel anywhere (the LDS-resident-W kernels, the split
// backward, no streaming head).  LHN_PW_K256=0: Cin = 256 in two K slices, the second accumulating into y.  LHN_PW_BWD_NARROW=0:
// 64 -> 64 and 32 -> 32 stay on k_pw_bwd.  LHN_PW_BWD_SPLIT=1: the wide shapes take lhn_pw_bwd_split.  LHN_HEAD_STREAM=0: the head
// stays on k_pw_fwd / k_pw_bwd + k_bias_grad_nchw and the plan runs every gate-gradient pass as its own launch.  All for A/B runs.
static unsigned pw_switches() {
  static int v = -1;
  if (v < 0) {
    const char *ld = getenv("LHN_PW_LDSW"), *k2 = getenv("LHN_PW_K256"), *na = getenv("LHN_PW_BWD_NARROW"), *sp = getenv("LHN_PW_BWD_SPLIT"),
               *hs = getenv("LHN_HEAD_STREAM");
    v = ((ld && ld[0] == '1') ? LHN_PW_SW_LDSW : 0) | ((k2 && k2[0] == '0') ? 0 : LHN_PW_SW_K256) |
        ((na && na[0] == '0') ? 0 : LHN_PW_SW_BWD_NARROW) | ((sp && sp[0] == '1') ? LHN_PW_SW_BWD_SPLIT : 0) |
        ((hs && hs[0] == '0') ? 0 : LHN_PW_SW_HEAD_STREAM) | (lhn_deterministic_mode() ? LHN_PW_SW_DETERMINISTIC : 0);
  }
  return (unsigned)v;
}
bool lhn_head_stream_on() { return (pw_switches() & LHN_PW_SW_HEAD_STREAM) != 0; }

// smallest tile width (16/32/64/128) that holds `c` input channels; 0 = none
static inline int pw_cin_tile(int c) { return c <= 16 ? 16 : c <= 32 ? 32 : c <= 64 ? 64 : c <= 128 ? 128 : 0; }
// 32-wide feature tiles per workgroup of the LDS-W kernels for `cc` features: 1, 2 or 4 (three run as four)
static inline int pw_feature_tiles(int cc) { return (cc + 31) / 32 == 3 ? 4 : (cc + 31) / 32; }
static inline bool pw_head_shape(const PwShape& s) { return lhn_head_shape(s.Cin, s.Cout, s.wcols, s.wrows); }
// reader-side BatchNorm sums: the k_pw_bwd tiles that have a BNS instance (the shapes the fused kernel keeps for itself)
constexpr bool pw_bwd_bns_tile(int ci, int nto) { return ci * nto * 32 < 64 * 128; }

// The slice at (co0, k0) of the sliced paths: cc features, kc input channels (kstep per launch) and the geometry its launch sees
struct PwSlice {
  int cc, kc;
  PwGeom g;
};
static PwSlice pw_slice(const PwShape& s, int kstep, int co0, int k0) {
  PwSlice t;
  t.cc = s.Cout - co0 < 128 ? s.Cout - co0 : 128;
  t.kc = s.Cin - k0 < kstep ? s.Cin - k0 : kstep;
  t.g = {s.wcols, s.wcols - k0 < t.kc ? s.wcols - k0 : t.kc, s.wrows - co0 < t.cc ? (s.wrows - co0 < 0 ? 0 : s.wrows - co0) : t.cc, 0, s.Cout, 0};
  return t;
}

// The register-W forward instances: `ci` input channels exactly, `cout` features, `ms` = summed-on-load sources.  K = 256
// (hourglassnet.py: every 1x1 of the C = 256 residuals) in ONE pass needs 128 features per block (64 would need 64-pixel tiles: 256
// VGPRs and spills).
static PwInst pw_wr_instance(int ci, int cout, bool ms) {
  const int ncot = cout <= 32 ? 1 : cout <= 64 ? 2 : 4;
  const bool ok = ms ? ((ci == 128 && ncot == 4) || (ci == 64 && ncot == 2))
                     : ci == 256 ? ncot == 4 : ci == 128 ? ncot >= 2 : (ci == 64 || ci == 32);
  return {ok ? ci : 0, ncot, ms ? 3 : 1, true, false};
}

// the forward launch of the slice at (co0, k0)
static PwInst pw_fwd_inst(const PwShape& s, unsigned sw, int kstep, int co0, int k0) {
  const PwSlice t = pw_slice(s, kstep, co0, k0);
  const int cc = t.cc, kc = t.kc, ci = kc == 256 ? 256 : pw_cin_tile(kc), nt = pw_feature_tiles(cc);
  const bool ms = s.f & (LHN_PW_F_EXTRA1 | LHN_PW_F_EXTRA2);
  // fast path: whole-K slice with full-width rows, plain NHWC store.  Slices of a C = 256 convolution qualify too: the kernel takes
  // the whole weight's row stride, accumulates later K slices into y and addresses the statistics of the whole BatchNorm.
  if (!(sw & LHN_PW_SW_LDSW) && s.stride == 1 && !(s.f & (LHN_PW_F_NCHW | LHN_PW_F_UNALIGNED)) && kc == ci && t.g.kvalid == ci && s.wcols % 4 == 0 &&
      t.g.wrows == cc) {
    PwInst i = pw_wr_instance(ci, cc, ms);
    // a finalize source rides in the two instances the narrow 1x1 -> depthwise chains reach, when one launch is the whole convolution
    i.fin = (s.f & LHN_PW_F_FINSRC) && !ms && s.Cin == ci && s.Cout <= 128 && ((ci == 64 && i.nt == 2) || (ci == 32 && i.nt == 1));
    if (i.ci) return i;
  }
  // summed-on-load sources: the square 1x1 of MSRB (litehourglass.py:30,49), C = 64 / 128
  if (ms) return {((ci == 128 && nt == 4) || (ci == 64 && nt == 2)) ? ci : 0, nt, 3, false, false};
  return {ci == 256 ? 0 : ci, nt, 1, false, false};
}

static PwRoute pw_fwd_route(const PwShape& s, unsigned sw) {
  PwRoute r = {PW_NONE, 128, LHN_PW_DGRAD_NONE, false, false, false, false, false};
  const bool nchw = s.f & LHN_PW_F_NCHW, ms = s.f & (LHN_PW_F_EXTRA1 | LHN_PW_F_EXTRA2), regw = !(sw & LHN_PW_SW_LDSW);
  const bool single = s.Cin <= 128 && s.Cout <= 128;
  r.finalize_in_front = s.f & LHN_PW_F_FINSRC;
  // the heatmap head (128 -> <= 32 features, NCHW, one source) on its streaming kernel; every other NCHW shape (H's stacked
  // 256 -> 21, padded heads, K slices) keeps k_pw_fwd
  if (nchw && (sw & LHN_PW_SW_HEAD_STREAM) && regw && s.stride == 1 && pw_head_shape(s) && !ms && !(s.f & (LHN_PW_F_SUM_OUT | LHN_PW_F_UNALIGNED)))
    return r.path = PW_HEAD, r;
  // (only summed-on-load sources can lack an instance, and they are one slice: every other slice has an LDS-W instance at least)
  if (ms && (!single || !pw_fwd_inst(s, sw, 128, 0, 0).ci)) return r;
  // Cin = 256 with full-width rows: the register-W kernel takes the whole K at once
  if ((sw & LHN_PW_SW_K256) && regw && s.Cin == 256 && s.wcols == 256 && s.stride == 1 && !nchw && !ms && s.Cout % 128 == 0 && s.wrows == s.Cout &&
      !(s.f & LHN_PW_F_UNALIGNED))
    r.kstep = 256;
  r.path = PW_SLICED;
  // a fused finalize rides in the kernel only when one launch is the whole convolution
  r.separate_finalize = !single && (s.f & LHN_PW_F_FUSE_FIN) && (s.f & LHN_PW_F_STATS);
  if (r.finalize_in_front && single && pw_fwd_inst(s, sw, r.kstep, 0, 0).fin) r.finalize_in_front = false;
  return r;
}

// input tile of a backward slice of kc channels (no 16-wide backward tile)
static inline int pw_bwd_cin_tile(int kc) { return kc <= 32 ? 32 : pw_cin_tile(kc); }

// The split path's instances: every slice must have one BEFORE anything is launched (dy is formed in place: no way back afterwards).
// Slices are all alike: channel counts above 128 must be multiples of 128.
static bool pw_split_route(const PwShape& s, unsigned sw, int* dgrad) {
  const LhnPwSplitTiles t = lhn_pw_split_tiles(s.Cin, s.Cout);
  const int cc = t.cc, kc = t.kc;
  const bool dx = !(s.f & LHN_PW_F_NO_DX), regw = !(sw & LHN_PW_SW_LDSW);
  if ((s.Cin > 128 && s.Cin % 128 != 0) || (s.Cout > 128 && s.Cout % 128 != 0)) return false;
  if ((dx && !lhn_pw_split_instance(cc, t.ntd)) || !lhn_pw_split_instance(kc, t.nto)) return false;
  *dgrad = !dx ? LHN_PW_DGRAD_NONE
           : (regw && s.Cout == 256 && pw_wr_instance(256, kc, false).ci) ? LHN_PW_DGRAD_WR256
           : (regw && (cc == 32 || cc == 64 || cc == 128) && pw_wr_instance(cc, kc, false).ci) ? LHN_PW_DGRAD_WR
                                                                                                : LHN_PW_DGRAD_KXK;
  return true;
}

static PwRoute pw_bwd_route(const PwShape& s, unsigned sw) {
  PwRoute r = {PW_NONE, 128, LHN_PW_DGRAD_NONE, false, false, false, false, false};
  const bool nchw = s.f & LHN_PW_F_NCHW, bns = s.f & LHN_PW_F_BNSUM, fin = s.f & LHN_PW_F_FIN, gs = s.f & LHN_PW_F_GATESUM;
  const bool regw = !(sw & LHN_PW_SW_LDSW);
  // reader-side BatchNorm sums ride in the fused kernel's BNS instances and in the narrow register-W ones (both inside the tile rule);
  // an NCHW gradient runs the NCHW instances, which take no sums: such a call is accepted by its channel product, as it always was
  if (bns && (s.stride != 1 || s.Cin > 128 || s.Cout > 128 || (s.f & LHN_PW_F_NO_DX) ||
              (nchw ? s.Cin * s.Cout >= 64 * 128 : !pw_bwd_bns_tile(pw_bwd_cin_tile(s.Cin), pw_feature_tiles(s.Cout)))))
    return r;
  // the heatmap head (128 -> <= 32 features from NCHW planes) on its streaming kernel: dx, dW, dbias and the gate sums of x's buffer
  // in ONE launch.  Gate sums only where a tile stays inside an image, and not in deterministic mode: an image's sums have several
  // writers there (dW and dbias have one writer per replica: at most 4 workgroups).
  if (nchw && (sw & LHN_PW_SW_HEAD_STREAM) && regw && s.stride == 1 && !bns && !fin && pw_head_shape(s) && s.HoWo % 4 == 0 &&
      !(s.f & LHN_PW_F_UNALIGNED) && (!gs || (s.HoWo % 64 == 0 && !(sw & LHN_PW_SW_DETERMINISTIC))))
    return r.path = PW_HEAD, r;
  const bool whole = s.stride == 1 && !nchw && s.wcols == s.Cin && s.wrows == s.Cout;
  if (whole && !bns && regw && !(sw & LHN_PW_SW_BWD_SPLIT) &&
      ((s.Cin == 128 && s.Cout == 128) || (s.Cin == 64 && s.Cout == 128) || (s.Cin == 128 && s.Cout == 64))) {
    r.path = PWB_WIDE;
    r.dyst = !(s.f & LHN_PW_F_DZ_DEAD);      // dz declared dead: dy stays in LDS
  } else if (whole && regw && (sw & LHN_PW_SW_BWD_NARROW) && s.Cin == s.Cout && (s.Cin == 64 || s.Cin == 32)) {
    // The BNS instances compile the gate on x out: they rely on the dispatcher's `!x->gate` condition for sums -- if that check is
    // ever relaxed, gated sums calls must leave this branch
    r.path = PWB_NARROW;
    r.bns = bns;
  } else if (whole && !bns && s.Cin * s.Cout >= 64 * 128 && s.Cout % 32 == 0 && s.Cin % 32 == 0 && s.Cout <= 256 && pw_split_route(s, sw, &r.dgrad)) {
    r.path = PWB_SPLIT;
  } else {
    r.path = PW_SLICED;
  }
  // the register-W instances fold the finalize in their prologue; every other path gets the separate launch, before its own first
  r.separate_finalize = fin && r.path != PWB_WIDE && r.path != PWB_NARROW;
  r.gate_reduce_after = gs;
  return r;
}

// =====================================================================================================
// Launch switches: from the route's instance to the template.
static int pw_fwd_launch(const PwInst& i, const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats, int stride,
                         float* y_nchw, int cout, const lhn_bnfin* fin, const PwGeom& geo, hipStream_t s, const PwExtra* ex, int wt = 0,
                         const lhn_bnfinsrc* fs = nullptr) {
  if (i.fin && fs) {
    if (i.ci == 64 && i.nt == 2) return launch_pw_fwd_wr<64, 2, 1, true>(x, w, bias, y, stats, cout, s, ex, geo, wt, stats ? fin : nullptr, fs);
    if (i.ci == 32 && i.nt == 1) return launch_pw_fwd_wr<32, 1, 1, true>(x, w, bias, y, stats, cout, s, ex, geo, wt, stats ? fin : nullptr, fs);
    LHN_CHECK_ARG(false, "lhn_conv_pw_fwd: no folding instance for %d channels x %d tiles", i.ci, i.nt);
  }
#define PW_KEY(WRV, CI, NTV, NSV) ((((WRV) * 1000 + (CI)) * 10 + (NTV)) * 10 + (NSV))
  switch (PW_KEY(i.wr, i.ci, i.nt, i.ns)) {
#define WR(CI, NC, NSV) case PW_KEY(1, CI, NC, NSV): return launch_pw_fwd_wr<CI, NC, NSV>(x, w, bias, y, stats, cout, s, ex, geo, wt, stats ? fin : nullptr);
    WR(256, 4, 1) WR(128, 4, 3) WR(64, 2, 3) WR(128, 4, 1) WR(128, 2, 1) WR(64, 4, 1) WR(64, 2, 1) WR(64, 1, 1) WR(32, 4, 1) WR(32, 2, 1) WR(32, 1, 1)
#undef WR
#define LW(CI, NTV, NSV) case PW_KEY(0, CI, NTV, NSV): return launch_pw_fwd<CI, NTV, NSV>(x, w, bias, y, stats, stride, y_nchw, cout, fin, geo, s, ex);
    LW(128, 4, 3) LW(64, 2, 3) LW(32, 1, 1) LW(32, 2, 1) LW(32, 4, 1) LW(64, 1, 1) LW(64, 2, 1) LW(64, 4, 1) LW(128, 1, 1) LW(128, 2, 1)
    LW(128, 4, 1) LW(16, 1, 1) LW(16, 2, 1) LW(16, 4, 1)
#undef LW
#undef PW_KEY
    default: LHN_CHECK_ARG(false, "lhn_conv_pw_fwd: no kernel instance for %d channels x %d tiles", i.ci, i.nt);
  }
}

int lhn_pw_dgrad_wr(const lhn_view* dyv, const float* w, const lhn_view* dxv, int wstride, int accumulate, hipStream_t s) {
  const PwGeom g = {wstride, dyv->C, dxv->C, accumulate, dxv->C, 0};
  return pw_fwd_launch(pw_wr_instance(dyv->C, dxv->C, false), dyv, w, nullptr, dxv, nullptr, 1, nullptr, dxv->C, nullptr, g, s, nullptr, 1);
}

// k_pw_bwd<CIN, NTO, NCHW, BNS>: the NCHW instances take no sums; the route has refused sums on a tile without a BNS instance
template <int CIN, int NTO>
static int launch_pw_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_acc,
                         float* dw, float* dbias, int stride, const float* dy_nchw, int cout, int nrep, int64_t rep_stride,
                         const PwGeom& geo, hipStream_t s, const lhn_bnsum& bs) {
  if (dy_nchw) return launch_pw_bwd_t<CIN, NTO, true>(x, w, y, gy, dx, dx_acc, dw, dbias, stride, dy_nchw, cout, nrep, rep_stride, geo, s, bs);
  if constexpr (pw_bwd_bns_tile(CIN, NTO)) {
    if (bs.sums) return launch_pw_bwd_t<CIN, NTO, false, true>(x, w, y, gy, dx, dx_acc, dw, dbias, stride, dy_nchw, cout, nrep, rep_stride, geo, s, bs);
  }
  return launch_pw_bwd_t<CIN, NTO, false>(x, w, y, gy, dx, dx_acc, dw, dbias, stride, dy_nchw, cout, nrep, rep_stride, geo, s, bs);
}

// The k_pw_bwd_wr instances: Cin, Cout, PX, PF, DYST, BNS, OCC.  Wide ones with and without the dy store, narrow ones with and without sums.
#define PW_BWD_WR_INSTANCES(X)                                                                                                  \
  X(128, 128, 32, 1, true, false, 2) X(128, 128, 32, 1, false, false, 2) X(64, 128, 64, 1, true, false, 2) X(64, 128, 64, 1, false, false, 2) \
  X(128, 64, 64, 2, true, false, 2) X(128, 64, 64, 2, false, false, 2) X(64, 64, 64, 2, false, false, 2) X(64, 64, 64, 2, false, true, 2)     \
  X(32, 32, 128, 2, false, false, 3) X(32, 32, 128, 2, false, true, 2)
#define PW_BWD_WR_KEY(CI, CO, DY, BN) ((((CI) * 1000 + (CO)) * 2 + ((DY) ? 1 : 0)) * 2 + ((BN) ? 1 : 0))

// =====================================================================================================
// Dispatchers: validate everything, ask the route, issue the separate finalize launch when the route says so, launch.
static int pw_fwd_run(const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats, int stride, float* y_nchw,
                      const lhn_bnfin* fin, const lhn_pw_opts* opts, const lhn_bnfinsrc* fsrc, void* stream) {
  if (fsrc && !fsrc->stats) fsrc = nullptr;
  if (fsrc)
    LHN_CHECK_ARG(lhn_view_ok(x) && !(opts && opts->n_extra > 0) && fsrc->table && fsrc->table == x->table && fsrc->cstride == x->cstride &&
                      fsrc->coff == x->coff && fsrc->C == x->C && fsrc->count >= 1 && (!fsrc->running_mean || fsrc->running_var),
                  "lhn_conv_pw_fwd: the finalize source must be the BatchNorm of x (its table and channel slice), one source");
  LHN_CHECK_ARG(lhn_view_ok(x) && w && y, "lhn_conv_pw_fwd: bad input view / null pointer");
  LHN_CHECK_ARG(stride == 1 || stride == 2, "lhn_conv_pw_fwd: stride %d", stride);
  LHN_CHECK_ARG(y->N == x->N && y->H == (x->H + stride - 1) / stride && y->W == (x->W + stride - 1) / stride,
                "lhn_conv_pw_fwd: output geometry %dx%dx%d does not match input %dx%dx%d / stride %d", y->N, y->H, y->W,
                x->N, x->H, x->W, stride);
  const int Cout = y->C, Cin = x->C, HoWo = y->H * y->W;
  if (y_nchw) {
    LHN_CHECK_ARG(HoWo % 4 == 0 && Cout > 0, "lhn_conv_pw_fwd: NCHW output needs H*W %% 4 == 0");
    LHN_CHECK_ARG(!stats, "lhn_conv_pw_fwd: no statistics on the NCHW head");
  } else {
    LHN_CHECK_ARG(lhn_view_ok(y), "lhn_conv_pw_fwd: bad output view");
  }
  LHN_CHECK_ARG((int64_t)y->N * y->H * y->W < (1ll << 31) - 256, "lhn_conv_pw_fwd: too many pixels");
  // weight tensor: [w_rows][w_cols], w_cols real input channels (<= Cin, the view may be padded to a multiple of 4),
  // w_rows real output features (<= Cout)
  const int wcols = (opts && opts->w_cols > 0) ? opts->w_cols : Cin, wrows = (opts && opts->w_rows > 0) ? opts->w_rows : Cout;
  LHN_CHECK_ARG(wcols <= Cin && wcols > Cin - 4 && wrows <= Cout, "lhn_conv_pw_fwd: weight [%d][%d] does not fit views %d -> %d",
                wrows, wcols, Cin, Cout);
  const int64_t bstride = (opts && opts->nchw_batch_stride > 0) ? opts->nchw_batch_stride : (int64_t)Cout * HoWo;
  const bool single = Cin <= 128 && Cout <= 128;
  PwExtra ex;
  ex.n = 0;
  ex.sum_out = nullptr;
  ex.so_cstride = ex.so_coff = 0;
  LHN_CHECK_ARG(lhn_no_pend(x), "lhn_conv_pw_fwd: lhn_view.pend is reserved (NULL)");
  if (opts && opts->n_extra > 0) {
    LHN_CHECK_ARG(opts->n_extra <= 2 && opts->extra && single && stride == 1, "lhn_conv_pw_fwd: extra sources need stride 1 and <= 128 channels");
    ex.n = opts->n_extra;
    for (int e = 0; e < ex.n; ++e) {
      const lhn_view* v = &opts->extra[e];
      LHN_CHECK_ARG(lhn_view_ok(v) && v->C == Cin && v->N == x->N && v->H == x->H && v->W == x->W && lhn_no_pend(v), "lhn_conv_pw_fwd: extra source %d geometry", e);
      ex.v[e] = *v;
    }
    for (int e = 0; e < 3; ++e) ex.coef[e] = opts->coef[e];
    if (opts->sum_out) {
      const lhn_view* so = opts->sum_out;
      LHN_CHECK_ARG(so->data && so->C == Cin && so->N == x->N && so->H == x->H && so->W == x->W && so->cstride % 4 == 0 && so->coff % 4 == 0 &&
                        so->coff + so->C <= so->cstride && Cout <= 128 && Cin % 4 == 0,
                    "lhn_conv_pw_fwd: sum_out geometry (same pixels and channels as x, one output slice)");
      ex.sum_out = so->data;
      ex.so_cstride = so->cstride;
      ex.so_coff = so->coff;
    }
  } else {
    LHN_CHECK_ARG(!(opts && opts->sum_out), "lhn_conv_pw_fwd: sum_out without extra sources");
  }
  const bool unaligned = (reinterpret_cast<uintptr_t>(w) & 15) != 0 || (y_nchw && ((reinterpret_cast<uintptr_t>(y_nchw) & 15) != 0 || bstride % 4 != 0));
  const PwShape sh = {x->N, x->H, x->W, HoWo, Cin, Cout, stride, wcols, wrows,
                      (y_nchw ? LHN_PW_F_NCHW : 0u) | (stats ? LHN_PW_F_STATS : 0u) | (fin ? LHN_PW_F_FUSE_FIN : 0u) |
                          (ex.n == 1 ? LHN_PW_F_EXTRA1 : ex.n == 2 ? LHN_PW_F_EXTRA2 : 0u) | (ex.sum_out ? LHN_PW_F_SUM_OUT : 0u) |
                          (unaligned ? LHN_PW_F_UNALIGNED : 0u) | (fsrc ? LHN_PW_F_FINSRC : 0u)};
  const unsigned sw = pw_switches();
  const PwRoute r = pw_fwd_route(sh, sw);
  LHN_CHECK_ARG(r.path != PW_NONE, "lhn_conv_pw_fwd: unsupported channels Cin=%d Cout=%d (%d extra sources)", Cin, Cout, ex.n);
  hipStream_t s = (hipStream_t)stream;
  int rc = 0;
  if (r.finalize_in_front)
    rc = lhn_bn_finalize(fsrc->stats, fsrc->gamma, fsrc->beta, fsrc->running_mean, fsrc->running_var, fsrc->num_batches_tracked, fsrc->table,
                         fsrc->cstride, fsrc->coff, fsrc->C, fsrc->save_mean_invstd, fsrc->count, fsrc->eps, fsrc->momentum, fsrc->slope, 1,
                         fsrc->conv_bias, stream);
  if (rc) return rc;
  rc = r.path == PW_HEAD ? lhn_head_fwd(x, w, bias, y_nchw, Cout, HoWo, bstride, s) : 0;
  for (int co0 = 0; r.path == PW_SLICED && co0 < Cout && !rc; co0 += 128) {
    for (int k0 = 0; k0 < Cin && !rc; k0 += r.kstep) {
      PwSlice t = pw_slice(sh, r.kstep, co0, k0);
      const bool last = k0 + t.kc >= Cin;
      lhn_view xv = *x, yv = *y;
      xv.coff += k0;
      xv.C = t.kc;
      if (!y_nchw) {
        yv.coff += co0;
        yv.C = t.cc;
      }
      t.g.yacc = k0 > 0;
      t.g.nchw_bstride = bstride;
      rc = pw_fwd_launch(pw_fwd_inst(sh, sw, r.kstep, co0, k0), &xv, w + (int64_t)co0 * wcols + k0, (last && bias) ? bias + co0 : nullptr,
                         &yv, (last && stats) ? stats + co0 : nullptr, stride, y_nchw ? y_nchw + (int64_t)co0 * HoWo : nullptr, t.cc,
                         single ? fin : nullptr, t.g, s, &ex, 0, r.finalize_in_front ? nullptr : fsrc);
    }
  }
  if (rc) return rc;
  LHN_CHECK_LAUNCH("lhn_conv_pw_fwd");
  if (r.separate_finalize)
    return lhn_bn_finalize(stats, fin->gamma, fin->beta, fin->running_mean, fin->running_var, fin->num_batches_tracked, fin->table,
                           fin->cstride, fin->coff, fin->C, fin->save_mean_invstd, fin->count, fin->eps, fin->momentum, fin->slope,
                           1, fin->conv_bias, stream);
  return 0;
}

// fin: the BatchNorm-backward finalize of y (lhn_bnbwdsrc).  gs: gate-gradient sums of x's buffer (lhn_gatesum): the caller finds the
// same sums whichever kernel ran.  flags: LHN_PW_BWD_DZ_DEAD.
static int pw_bwd_run(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate, float* dw,
                      float* dbias, int stride, const float* dy_nchw, int nrep, int64_t rep_stride, const lhn_pw_opts* opts,
                      const lhn_bnsum* bns, const lhn_bnbwdsrc* fin, const lhn_gatesum* gs, int flags, void* stream) {
  static const char* const sums_text =
      "lhn_conv_pw_bwd3: BatchNorm sums ride in the fused kernel only (stride 1, a stored dx, Cin and Cout <= 128 in tiles below 64 x 128, ungated input inside the producer's channels)";
  if (gs && !gs->dgate) gs = nullptr;
  // (dx accumulated: the head kernel would sum this call's part of dx, the reduce launch the whole buffer -- refused, so the
  // result cannot depend on the route; the executor only ever passes the stored mode)
  if (gs) LHN_CHECK_ARG(lhn_view_ok(x) && dx && !dx_accumulate && stride == 1 && (!gs->slices || (gs->slices->n >= 0 && gs->slices->n <= 2)),
                        "lhn_conv_pw_bwd5: gate sums need a stored dx (no accumulate), stride 1 and 0..2 BatchNorm slices");
  if (nrep < 1) nrep = 1;
  if (fin && !fin->sums) fin = nullptr;
  lhn_bnsum bs;
  memset(&bs, 0, sizeof(bs));
  if (bns && bns->sums) {
    LHN_CHECK_ARG(x && y && bns->save && dx && stride == 1 && x->C <= 128 && y->C <= 128 && !x->gate && x->table && bns->coff >= 0 &&
                      bns->coff + x->C <= bns->C,
                  "%s", sums_text);
    bs = *bns;
  }
  LHN_CHECK_ARG(lhn_view_ok(x) && w && y && gy && dw && lhn_no_pend(x) && lhn_no_pend(y), "lhn_conv_pw_bwd: bad view / null pointer");
  LHN_CHECK_ARG(stride == 1 || stride == 2, "lhn_conv_pw_bwd: stride %d", stride);
  LHN_CHECK_ARG(stride == 1 || !dx || dx_accumulate, "lhn_conv_pw_bwd: stride-2 dgrad only accumulates into a zeroed gradient");
  if (!dy_nchw) LHN_CHECK_ARG(lhn_view_ok(y) && gy->dz, "lhn_conv_pw_bwd: bad output view / missing dz");
  const int Cout = y->C, Cin = x->C, HoWo = y->H * y->W;
  const int wcols = (opts && opts->w_cols > 0) ? opts->w_cols : Cin, wrows = (opts && opts->w_rows > 0) ? opts->w_rows : Cout;
  LHN_CHECK_ARG(wcols <= Cin && wcols > Cin - 4 && wrows <= Cout, "lhn_conv_pw_bwd: weight [%d][%d] does not fit views %d -> %d",
                wrows, wcols, Cin, Cout);
  const int64_t bstride = (opts && opts->nchw_batch_stride > 0) ? opts->nchw_batch_stride : (int64_t)Cout * HoWo;
  if (fin)
    LHN_CHECK_ARG(!dy_nchw && gy->coef && fin->save_mean_invstd && fin->count > 0 && fin->stat_channels >= Cout,
                  "lhn_conv_pw_bwd4: finalize source needs gy->coef, saved statistics and stat_channels >= Cout");
  const bool unaligned = dy_nchw && (bstride % 4 != 0 || ((reinterpret_cast<uintptr_t>(dy_nchw) | reinterpret_cast<uintptr_t>(x->data)) & 15) != 0);
  const PwShape sh = {x->N, x->H, x->W, HoWo, Cin, Cout, stride, wcols, wrows,
                      (dy_nchw ? LHN_PW_F_NCHW : 0u) | (bs.sums ? LHN_PW_F_BNSUM : 0u) | (fin ? LHN_PW_F_FIN : 0u) | (gs ? LHN_PW_F_GATESUM : 0u) |
                          (dx ? 0u : LHN_PW_F_NO_DX) | (dx_accumulate ? LHN_PW_F_DX_ACC : 0u) | ((flags & LHN_PW_BWD_DZ_DEAD) ? LHN_PW_F_DZ_DEAD : 0u) |
                          (dbias ? LHN_PW_F_DBIAS : 0u) | (unaligned ? LHN_PW_F_UNALIGNED : 0u)};
  const PwRoute r = pw_bwd_route(sh, pw_switches());
  LHN_CHECK_ARG(r.path != PW_NONE, "%s", sums_text);      // (the sums are what has no instance everywhere)
  if (r.separate_finalize) {
    const int rc = lhn_bn_bwd_finalize2(fin->sums, fin->gamma, fin->save_mean_invstd, const_cast<float*>(gy->coef), y->cstride, y->coff,
                                        Cout, fin->stat_channels, fin->count, fin->dgamma, fin->dbeta, fin->pgrad_scale, stream);
    if (rc) return rc;
    fin = nullptr;
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = 0;
  switch (r.path) {
    case PW_HEAD: rc = lhn_head_bwd(x, w, dy_nchw, dx, dx_accumulate, dw, dbias, Cout, HoWo, bstride, nrep, rep_stride, gs, s); break;
    case PWB_WIDE:
    case PWB_NARROW:
      switch (PW_BWD_WR_KEY(Cin, Cout, r.dyst, r.bns)) {
#define X(CI, CO, PXV, PFV, DY, BN, OC) \
  case PW_BWD_WR_KEY(CI, CO, DY, BN): rc = launch_pw_bwd_wr<CI, CO, PXV, PFV, DY, BN, OC>(x, w, y, gy, dx, dx_accumulate, dw, dbias, nrep, rep_stride, s, bs, fin); break;
        PW_BWD_WR_INSTANCES(X)
#undef X
      }
      break;
    case PWB_SPLIT: rc = lhn_pw_bwd_split(x, w, y, gy, dx, dx_accumulate, dw, dbias, nrep, rep_stride, r.dgrad, s); break;
    default:
      for (int co0 = 0; co0 < Cout && !rc; co0 += 128) {
        for (int k0 = 0; k0 < Cin && !rc; k0 += 128) {
          PwSlice t = pw_slice(sh, 128, co0, k0);
          lhn_view xv = *x, yv = *y;
          xv.coff += k0;
          xv.C = t.kc;
          if (!dy_nchw) {
            yv.coff += co0;
            yv.C = t.cc;
          }
          t.g.nchw_bstride = bstride;
          const float* wv = w + (int64_t)co0 * wcols + k0;
          float* dwv = dw + (int64_t)co0 * wcols + k0;
          float* dbv = (dbias && k0 == 0) ? dbias + co0 : nullptr;
          const float* dyv = dy_nchw ? dy_nchw + (int64_t)co0 * HoWo : nullptr;
          const int acc = dx_accumulate || co0 > 0;
          switch (pw_bwd_cin_tile(t.kc) * 10 + pw_feature_tiles(t.cc)) {
#define PWB_CASE(CI, NTV) \
  case CI * 10 + NTV: rc = launch_pw_bwd<CI, NTV>(&xv, wv, &yv, gy, dx, acc, dwv, dbv, stride, dyv, t.cc, nrep, rep_stride, t.g, s, bs); break;
            PWB_CASE(32, 1) PWB_CASE(32, 2) PWB_CASE(32, 4) PWB_CASE(64, 1) PWB_CASE(64, 2) PWB_CASE(64, 4) PWB_CASE(128, 1)
            PWB_CASE(128, 2) PWB_CASE(128, 4)
#undef PWB_CASE
          }
        }
      }
  }
  if (rc) return rc;
  LHN_CHECK_LAUNCH("lhn_conv_pw_bwd");
  if (!r.gate_reduce_after) return 0;
  lhn_view xv = *x;
  xv.gate = nullptr;
  return lhn_gate_bwd_reduce3(&xv, dx, gs->dgate, gs->dgate + (size_t)x->N * x->cstride, gs->slices, 1, stream);
}

// =====================================================================================================
// Entry points.  The numbered forms differ in what a call may carry; each forwards to the widest.
extern "C" int lhn_conv_pw_fwd(const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats,
                               int stride, float* y_nchw, const lhn_bnfin* fin, void* stream) {
  return lhn_conv_pw_fwd2(x, w, bias, y, stats, stride, y_nchw, fin, nullptr, stream);
}
extern "C" int lhn_conv_pw_fwd2(const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats,
                                int stride, float* y_nchw, const lhn_bnfin* fin, const lhn_pw_opts* opts, void* stream) {
  return pw_fwd_run(x, w, bias, y, stats, stride, y_nchw, fin, opts, nullptr, stream);
}
extern "C" int lhn_conv_pw_fwd3(const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats,
                                int stride, float* y_nchw, const lhn_bnfin* fin, const lhn_pw_opts* opts, const lhn_bnfinsrc* finsrc,
                                void* stream) {
  return pw_fwd_run(x, w, bias, y, stats, stride, y_nchw, fin, opts, finsrc, stream);
}
extern "C" int lhn_conv_pw_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                               int dx_accumulate, float* dw, float* dbias, int stride, const float* dy_nchw, int nrep,
                               int64_t rep_stride, void* stream) {
  return lhn_conv_pw_bwd6(x, w, y, gy, dx, dx_accumulate, dw, dbias, stride, dy_nchw, nrep, rep_stride, nullptr, nullptr, nullptr, nullptr, 0, stream);
}
extern "C" int lhn_conv_pw_bwd2(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, float* dbias, int stride, const float* dy_nchw, int nrep,
                                int64_t rep_stride, const lhn_pw_opts* opts, void* stream) {
  return lhn_conv_pw_bwd6(x, w, y, gy, dx, dx_accumulate, dw, dbias, stride, dy_nchw, nrep, rep_stride, opts, nullptr, nullptr, nullptr, 0, stream);
}
extern "C" int lhn_conv_pw_bwd3(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, float* dbias, int stride, const float* dy_nchw, int nrep,
                                int64_t rep_stride, const lhn_pw_opts* opts, const lhn_bnsum* bns, void* stream) {
  return lhn_conv_pw_bwd6(x, w, y, gy, dx, dx_accumulate, dw, dbias, stride, dy_nchw, nrep, rep_stride, opts, bns, nullptr, nullptr, 0, stream);
}
extern "C" int lhn_conv_pw_bwd4(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, float* dbias, int stride, const float* dy_nchw, int nrep,
                                int64_t rep_stride, const lhn_pw_opts* opts, const lhn_bnsum* bns, const lhn_bnbwdsrc* fin, void* stream) {
  return lhn_conv_pw_bwd6(x, w, y, gy, dx, dx_accumulate, dw, dbias, stride, dy_nchw, nrep, rep_stride, opts, bns, fin, nullptr, 0, stream);
}
extern "C" int lhn_conv_pw_bwd5(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, float* dbias, int stride, const float* dy_nchw, int nrep,
                                int64_t rep_stride, const lhn_pw_opts* opts, const lhn_bnsum* bns, const lhn_bnbwdsrc* fin,
                                const lhn_gatesum* gs, void* stream) {
  return lhn_conv_pw_bwd6(x, w, y, gy, dx, dx_accumulate, dw, dbias, stride, dy_nchw, nrep, rep_stride, opts, bns, fin, gs, 0, stream);
}
extern "C" int lhn_conv_pw_bwd6(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, float* dbias, int stride, const float* dy_nchw, int nrep,
                                int64_t rep_stride, const lhn_pw_opts* opts, const lhn_bnsum* bns, const lhn_bnbwdsrc* fin,
                                const lhn_gatesum* gs, int flags, void* stream) {
  return pw_bwd_run(x, w, y, gy, dx, dx_accumulate, dw, dbias, stride, dy_nchw, nrep, rep_stride, opts, bns, fin, gs, flags, stream);
}

// Host only: the names of what pw_fwd_run / pw_bwd_run would launch, in order (include/lhn.h).
extern "C" const char* lhn_conv_pw_route(int backward, int N, int H, int W, int Cin, int Cout, int stride, int w_rows, int w_cols,
                                         int features, int switches) {
  if (stride != 1 && stride != 2) return nullptr;
  const PwShape sh = {N, H, W, ((H + stride - 1) / stride) * ((W + stride - 1) / stride), Cin, Cout, stride, w_cols > 0 ? w_cols : Cin,
                      w_rows > 0 ? w_rows : Cout, (unsigned)features};
  const unsigned sw = switches < 0 ? pw_switches() : (unsigned)switches;
  const PwRoute r = (backward ? pw_bwd_route : pw_fwd_route)(sh, sw);
  if (r.path == PW_NONE) return nullptr;
  static thread_local char buf[768];
  size_t len = 0;
  char run[96] = "", cur[96];
  int reps = 0;
  auto flush = [&] {      // the pending name, " x n" for a repeated launch
    if (!reps) return;
    len += snprintf(buf + len, sizeof(buf) - len, reps > 1 ? "%s%s x %d" : "%s%s", len ? " + " : "", run, reps);
    if (len >= sizeof(buf)) len = sizeof(buf) - 1;
    reps = 0;
  };
  auto emit = [&](const char* name) {
    if (reps && strcmp(run, name) != 0) flush();
    snprintf(run, sizeof(run), "%s", name);
    ++reps;
  };
  auto fwd_name = [&](const PwInst& i) {
    snprintf(cur, sizeof(cur), i.fin ? "%s<%d, %d, %d, true>" : "%s<%d, %d, %d>", i.wr ? "k_pw_fwd_wr" : "k_pw_fwd", i.ci, i.nt, i.ns);
    emit(cur);
  };
  const char* const tf[] = {"false", "true"};
  buf[0] = 0;
  if (r.separate_finalize && backward) emit("lhn_bn_bwd_finalize2");
  if (r.finalize_in_front && !backward) emit("lhn_bn_finalize");
  switch (r.path) {
    case PW_HEAD:
      snprintf(cur, sizeof(cur), "k_head_bwd<%s>", tf[(features & LHN_PW_F_GATESUM) != 0]);
      emit(backward ? cur : "k_head_fwd");
      break;
    case PWB_WIDE:
    case PWB_NARROW:
      switch (PW_BWD_WR_KEY(Cin, Cout, r.dyst, r.bns)) {
#define X(CI, CO, PXV, PFV, DY, BN, OC) case PW_BWD_WR_KEY(CI, CO, DY, BN): emit("k_pw_bwd_wr<" #CI ", " #CO ", " #PXV ", " #PFV ", " #DY ", " #BN ", " #OC ">"); break;
        PW_BWD_WR_INSTANCES(X)
#undef X
      }
      break;
    case PWB_SPLIT: {
      emit("k_dy_inplace");
      const LhnPwSplitTiles t = lhn_pw_split_tiles(Cin, Cout);      // what lhn_pw_bwd_split launches from
      const int nco = r.dgrad == LHN_PW_DGRAD_WR256 ? 1 : t.nco;
      for (int j = 0; r.dgrad != LHN_PW_DGRAD_NONE && j < nco * (r.dgrad == LHN_PW_DGRAD_KXK ? 1 : t.nk); ++j) {
        if (r.dgrad == LHN_PW_DGRAD_KXK) {
          snprintf(cur, sizeof(cur), "k_kxk<%d, %d, 1, 1, true>", t.cc, t.ntd);
          emit(cur);
        } else {
          fwd_name(pw_wr_instance(r.dgrad == LHN_PW_DGRAD_WR256 ? 256 : t.cc, t.kc, false));
        }
      }
      snprintf(cur, sizeof(cur), "k_kxk_wgrad<%d, %d, 1, true>", t.kc, t.nto);
      for (int j = 0; j < t.nk; ++j) emit(cur);
      break;
    }
    default:
      for (int co0 = 0; co0 < Cout; co0 += 128)
        for (int k0 = 0; k0 < Cin; k0 += r.kstep) {
          if (!backward) {
            fwd_name(pw_fwd_inst(sh, sw, r.kstep, co0, k0));
            continue;
          }
          const PwSlice t = pw_slice(sh, 128, co0, k0);
          const bool nchw = features & LHN_PW_F_NCHW;
          snprintf(cur, sizeof(cur), "k_pw_bwd<%d, %d, %s, %s>", pw_bwd_cin_tile(t.kc), pw_feature_tiles(t.cc), tf[nchw], tf[!nchw && (features & LHN_PW_F_BNSUM)]);
          emit(cur);
          if (nchw && k0 == 0 && (features & LHN_PW_F_DBIAS)) emit("k_bias_grad_nchw");
        }
  }
  if (r.separate_finalize && !backward) emit("lhn_bn_finalize");
  if (r.gate_reduce_after) emit("lhn_gate_bwd_reduce3");
  flush();
  return buf;
}
