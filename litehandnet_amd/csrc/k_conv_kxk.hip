// Dense 3x3 convolution (pad 1, stride 1/2) as an fp32-MFMA implicit GEMM, NHWC:
//     Y[m][co] = sum_tap sum_ci X[m shifted by tap][ci] * W[co][ci][tap]
// i.e. nine accumulated shifted pointwise GEMMs (liteHandNet.py:23-54 BasicBlock / BottleNeck, :183 stem).
// MODE 0 forward : A = consumed input value (pending BN/act applied on load), epilogue = raw store + BN statistics
// MODE 1 dgrad   : A = dy formed on the fly from (dz, saved raw y, BN-backward coefficients), B = W^T with the
//                  taps mirrored, epilogue = dx store / accumulate
// wgrad          : one tap per blockIdx.y, dW_tap[co][ci] += dY^T X_shifted in registers across the block's tiles.
// Tile geometry, LDS images (+4 float row pad) and fragment maps are those of k_conv_pw.hip.
#include <stdlib.h>
#include "lhn_common.h"

// dz := dy in place (dy = A*du + B*y + C with du from gate / pooled gradient / leaky derivative).  Used ahead of the
// MFMA-heavy backward kernels: they then stream ONE plain tensor instead of (dz, raw y) + the formula per element,
// which halves their prefetch registers (no spills) -- worth one extra elementwise pass when Cin*Cout is large.
__global__ void __launch_bounds__(256) k_dy_inplace(lhn_view y, lhn_gradview g, float* __restrict__ dz, float* __restrict__ dbias,
                                                    int nrep, int64_t rep_stride) {
  __shared__ f4 red[256];
  const int C4 = y.C >> 2, c4 = threadIdx.x % C4, pl = threadIdx.x / C4, PL = 256 / C4;
  const int ca = y.coff + 4 * c4;
  const Xf4 xf = lhn_load_xf(y, ca);
  const Gr4 gr = lhn_load_coef(g, y.cstride, ca);
  const int rows = y.N * y.H;
  f4 bsum = (f4){0.f, 0.f, 0.f, 0.f};
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int n = row / y.H, h = row - n * y.H;
    for (int w = LHN_LANE0(pl, PL); w < y.W; w += PL) {
      const size_t off = ((size_t)row * y.W + w) * y.cstride + ca;
      const f4 raw = *reinterpret_cast<const f4*>(y.data + off);
      const f4 du = lhn_grad_du(y, g, xf, raw, *reinterpret_cast<const f4*>(dz + off), n, h, w, ca);
      const f4 dy = gr.A * du + gr.B * raw + gr.Cc;
      *reinterpret_cast<f4*>(dz + off) = dy;
      bsum += dy;
    }
  }
  // d(bias) of a biased convolution = column sums of dy: this pass already touches every element.  One thread per CHANNEL
  // adds its column (consecutive lanes -> consecutive addresses: the full-rate atomic form) into this block's gradient replica.
  if (dbias) {
    red[threadIdx.x] = bsum;                 // (lanes beyond PL * C4 never entered the loop: zero)
    __syncthreads();
    if ((int)threadIdx.x < y.C) {
      const float* rf = reinterpret_cast<const float*>(red);
      const int cc = threadIdx.x >> 2, jj = threadIdx.x & 3;
      float v = 0.f;
      for (int j = 0; j < PL; ++j) v += rf[(j * C4 + cc) * 4 + jj];
      atomicAdd(dbias + (size_t)(blockIdx.x % nrep) * rep_stride + threadIdx.x, v);
    }
  }
}
static void launch_dy_inplace(const lhn_view* y, const lhn_gradview* gy, hipStream_t s, float* dbias = nullptr, int nrep = 1,
                              int64_t rep_stride = 0) {
  int64_t g = (int64_t)y->N * y->H;
  const int64_t cap = (int64_t)lhn_num_cus() * 8;
  if (g > cap) g = cap;
  hipLaunchKernelGGL(k_dy_inplace, dim3((int)g), dim3(256), 0, s, *y, *gy, const_cast<float*>(gy->dz), dbias, nrep < 1 ? 1 : nrep, rep_stride);
}

// ---------------------------------------------------------------------------------------------------------
// Core.  GEMM rows = 128 pixels per tile (wave w owns rows [32w, 32w+32)), N = 32*NT features, one PHASE =
// one tap with the whole K = KD: 16*NT*KD/32... MFMAs per wave, long enough to cover memory latency with a single
// 4-wave workgroup per CU.  While a phase multiplies out of LDS, the A rows of the NEXT phase are already in
// flight into registers (raw loads; the pending BN/activation/gate or the dy formula is applied when they are
// committed to LDS after the MFMA loop).  Weights of the next tap are fetched at the start of the commit; for
// 1x1 (TAPS = 1) they are staged once per block.
// KD = 256 does not fit LDS whole (the A tile alone would be 133 KB): it runs as NSL = 2 slices of KW = 128 channels, a phase is
// then (tap, slice) -- 18 per tile -- on the LDS images and the MFMA loop of the <128, NT> instance, into the same accumulators.
// The per-thread channel offset and the pending transform belong to a slice: issue() sets them for the phase it loads.
// KD = 160 (mynet at width 160) runs the same way as NSL = 5 slices of KW = 32 on the images of the <32, NT> instance: 45 phases.
// KD = 40 (its quarter) is no multiple of 32: it runs on the 64-channel images with channels [40, 64) committed as zeros.  The
// lanes of that tail issue no A load in the forward and the plain data gradient (dy on the fly: a load clamped to channel 0, value
// discarded, which measured faster there); their table, gate, coefficient and tap-major weight loads are clamped to channel 0 and
// the weights staged as zeros.  The MFMA loop stops at the last group of 8 channels that holds a real one (5 of 8 at K = 40).
constexpr int kxk_kp(int kd) { return kd == 40 ? 64 : kd; }                                  // channels of the LDS images
constexpr int kxk_kw(int kd) { return kd == 160 ? 32 : kd > 128 ? 128 : kxk_kp(kd); }        // K slice held in LDS
template <int KD, int NT, int MODE, int TAPS, bool PLAIN = false>
__global__ void __launch_bounds__(256) k_kxk(lhn_view x, const float* __restrict__ w, lhn_view y, lhn_gradview gy,
                                             double* __restrict__ stats, float* __restrict__ dx, int dx_acc, int stride,
                                             int nout, int Mhost, int ntiles, lhn_bnfin fin, const float* __restrict__ wt) {
  constexpr int KW = kxk_kw(KD), NSL = (KD + KW - 1) / KW;   // K slice held in LDS, slices per tap
  constexpr bool KPAD = NSL * KW != KD;                      // channels [KD, NSL * KW) of the (last slice's) images are zeros
  static_assert(!KPAD || TAPS == 9, "padded K: 3x3 only");
  static_assert(NSL == 1 || (TAPS == 9 && (MODE == 0 || PLAIN)), "sliced K: 3x3 forward and plain dgrad only");
  constexpr int BM = 128, LDA = KW + 4;
  constexpr int C4 = KW / 4, RP = 256 / C4, PF = BM / RP;     // float4 per thread per phase
  constexpr int NW = 32 * NT * KW / 256;                      // weight scalars per thread per phase
  constexpr int WCH = NW > 16 ? (NW % 16 ? 10 : 16) : NW;     // staged in chunks of <= 16 registers (NT = 5: 20 = 2 x 10)
  static_assert(NW % WCH == 0, "whole chunks: a partial one would run past the W image");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ws = smem;                   // [32*NT][LDA]
  float* As = smem + 32 * NT * LDA;   // [128][LDA]
  float* red = As + BM * LDA;         // [4][32*NT][2]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int c4 = tid % C4, row0 = tid / C4;
  const int n0 = blockIdx.y * 32 * NT;        // N split: this block's first output feature (small M: more blocks)
  const lhn_view& av = MODE == 0 ? x : y;
  const lhn_view& ov = MODE == 0 ? y : x;
  // Stride-2 dgrad by input-pixel PARITY (gridDim.z == 4): an input pixel (ih, iw) only meets the taps with
  // kh = ih+1 (mod 2), kw = iw+1 (mod 2) -- 1, 2, 2 or 4 of the 9 -- so each parity class is its own small implicit GEMM
  // over its quarter of the pixels and its own tap list (2.25 taps per pixel on average instead of 9, 3/4 of them zeros).
  const bool par = (MODE == 1 && TAPS == 9 && gridDim.z == 4);
  const int ph = par ? (int)(blockIdx.z >> 1) : 0, pw2 = par ? (int)(blockIdx.z & 1) : 0;
  const int OH2 = par ? (ov.H - ph + 1) / 2 : ov.H, OW = par ? (ov.W - pw2 + 1) / 2 : ov.W, OHW = OH2 * OW;
  const int M = par ? ov.N * OHW : Mhost;
  const int nkw = (par && !pw2) ? 1 : (par ? 2 : 3), ntaps = par ? (ph ? 2 : 1) * nkw : TAPS;
  auto tap_of = [&](int t) __attribute__((always_inline)) -> int {
    if (!par) return t;
    const int a = t / nkw, b = t - a * nkw;
    return (ph ? 2 * a : 1) * 3 + (pw2 ? 2 * b : 1);
  };
  const int cin_total = MODE == 0 ? KD : nout;
  const int cabs0 = av.coff + ((!KPAD || 4 * c4 < KD) ? 4 * c4 : 0);      // (a lane of the zero tail: channel 0, see issue())
  const Xf4 xf0 = lhn_load_xf(av, cabs0);
  int cabs_s = cabs0;               // NSL > 1: offset and transform of the slice whose loads are in flight
  Xf4 xf_s = xf0;
  const int& cabs = NSL > 1 ? cabs_s : cabs0;
  const Xf4& xf = NSL > 1 ? xf_s : xf0;
  Gr4 gr;
  if (MODE == 1) gr = lhn_load_coef(gy, y.cstride, cabs);
  double ssum[NT], ssq[NT];          // per-tile fp32 partials promoted to double (see k_conv_pw.hip)
#pragma unroll
  for (int j = 0; j < NT; ++j) ssum[j] = ssq[j] = 0.0;

  constexpr bool LIN = (TAPS == 1);        // 1x1: launched with stride 1 only -> rows are linear pixel indices
  int rn[LIN ? 1 : PF], rh[LIN ? 1 : PF], rw[LIN ? 1 : PF];
  f4 pa[PF], pb[(MODE == 1 && !PLAIN) ? PF : 1];
  bool pv[PF];
  int cur_tile = 0;

  auto geom = [&](int tile) __attribute__((always_inline)) {
    cur_tile = tile;
    if (LIN) return;
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      // branch-free (an if/else over these small arrays made the compiler keep them in scratch memory)
      const int m = tile * BM + row0 + p * RP, mc = min(m, M - 1);
      const int n = mc / OHW, r = mc - n * OHW, i2 = r / OW, j2 = r - i2 * OW;
      rn[p] = m < M ? n : -1;
      rh[p] = par ? 2 * i2 + ph : i2;
      rw[p] = par ? 2 * j2 + pw2 : j2;
    }
  };
  auto issue = [&](int tap, int sl) __attribute__((always_inline)) {
    const int kh = TAPS == 1 ? 1 : tap / 3, kw = TAPS == 1 ? 1 : tap - (tap / 3) * 3;
    // padded K: whether this lane's four channels exist in the slice; a lane of the zero tail issues no load and commits zeros
    const bool cok = !KPAD || sl * KW + 4 * c4 < KD;
    if (NSL > 1) {       // the previous phase is committed: its offset and transform are dead
      cabs_s = KPAD ? av.coff + (cok ? sl * KW + 4 * c4 : 0) : cabs0 + sl * KW;
      if (MODE == 0) xf_s = lhn_load_xf(av, cabs_s);
    }
    if (LIN) {
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        const int m = cur_tile * BM + row0 + p * RP;
        pv[p] = m < M;
        const size_t off = (size_t)min(m, M - 1) * av.cstride + cabs;
        if (MODE == 1 && PLAIN) pa[p] = *reinterpret_cast<const f4*>(gy.dz + off);
        else pa[p] = *reinterpret_cast<const f4*>(av.data + off);
        if (MODE == 1 && !PLAIN) pb[(MODE == 1 && !PLAIN) ? p : 0] = *reinterpret_cast<const f4*>(gy.dz + off);
      }
      return;
    }
    if (KPAD && (MODE == 0 || PLAIN) && !cok) {      // (at K = 40 that is 6 lanes of 16: a third of the A traffic)
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        pv[p] = false;
        pa[p] = (f4){0.f, 0.f, 0.f, 0.f};
        if (MODE == 1 && !PLAIN) pb[(MODE == 1 && !PLAIN) ? p : 0] = (f4){0.f, 0.f, 0.f, 0.f};
      }
      return;
    }
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      // clamped, always-valid addresses: all loads of the phase issue back to back; validity is a select at commit
      const int n = rn[p] < 0 ? 0 : rn[p];
      if (MODE == 0) {
        const int ih = rh[p] * stride - 1 + kh, iw = rw[p] * stride - 1 + kw;
        const int ihc = min(max(ih, 0), x.H - 1), iwc = min(max(iw, 0), x.W - 1);
        pv[p] = cok && rn[p] >= 0 && ih == ihc && iw == iwc;
        pa[p] = *reinterpret_cast<const f4*>(x.data + ((size_t)(n * x.H + ihc) * x.W + iwc) * x.cstride + cabs);
      } else {
        const int hn = rh[p] + 1 - kh, wn2 = rw[p] + 1 - kw;
        const int ho = hn / stride, wo = wn2 / stride;     // hn, wn2 >= -1: trunc == floor where it matters (validity below)
        const int hoc = min(max(ho, 0), y.H - 1), woc = min(max(wo, 0), y.W - 1);
        pv[p] = cok && rn[p] >= 0 && hn >= 0 && wn2 >= 0 && ho * stride == hn && wo * stride == wn2 && ho == hoc && wo == woc;
        const size_t off = ((size_t)(n * y.H + hoc) * y.W + woc) * y.cstride + cabs;
        if (PLAIN) pa[p] = *reinterpret_cast<const f4*>(gy.dz + off);
        else {
          pa[p] = *reinterpret_cast<const f4*>(y.data + off);
          pb[(MODE == 1 && !PLAIN) ? p : 0] = *reinterpret_cast<const f4*>(gy.dz + off);
        }
      }
    }
  };
  auto stage_w = [&](int tap, int sl) __attribute__((always_inline)) {
    if (TAPS > 1 && wt) {
      // tap-major copy of the weights (k_w_tapmajor): row = output feature of this GEMM, KD contiguous floats per row ->
      // 16-byte loads/stores instead of 4-byte gathers with a 36-byte stride (which cost more than the MFMAs of a phase).
      // A slice takes KW of a row's KD floats, from sl * KW.
      constexpr int NWV = 32 * NT * KW / 4 / 256, K4 = KW / 4;
      // NWV < 4 (32 * NT * KD < 4096): the fixed group of four below runs past the W image, and vector j >= NWV of thread tid
      // lands in As at exactly the slot that commit() writes for p = j - NWV of the SAME thread (both map the linear index
      // tid + 256 * j to (row, k4) the same way, and 32 * NT * K4 == 256 * NWV).  commit() always follows stage_w() before the
      // barrier, so the stray value is overwritten in program order by its own thread: in bounds (j - NWV < PF), no effect.
      // That holds only while the two mappings stay equal -- change either and this becomes an LDS write-write race
      // between waves; bound the loop by NWV then.  (Slices of 128 have NWV >= 4: nothing runs past.  Slices of 32 and the padded
      // 40 are the <32, NT> and <64, NT> images with their mappings.  NT = 5: NWV = 5, the second group of four runs three past.)
#pragma unroll
      for (int j0 = 0; j0 < NWV; j0 += 4) {
        f4 t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = tid + 256 * (j0 + j), nn = i / K4, k4 = i - nn * K4;
          t[j] = *reinterpret_cast<const f4*>(wt + ((size_t)tap * nout + min(n0 + nn, nout - 1)) * KD + sl * KW + (KPAD && sl * KW + 4 * k4 >= KD ? 0 : 4 * k4));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = tid + 256 * (j0 + j), nn = i / K4, k4 = i - nn * K4;
          *reinterpret_cast<f4*>(Ws + nn * LDA + 4 * k4) = (n0 + nn < nout && (!KPAD || sl * KW + 4 * k4 < KD)) ? t[j] : (f4){0.f, 0.f, 0.f, 0.f};
        }
      }
      return;
    }
#pragma unroll 1
    for (int j0 = 0; j0 < NW; j0 += WCH) {
      float t[WCH];
#pragma unroll
      for (int j = 0; j < WCH; ++j) {
        const int i = tid + 256 * (j0 + j);
        float v = 0.f;
        if (MODE == 0 || TAPS > 1) {
          const int nn = i / KW, kk = i - nn * KW, ka = sl * KW + kk;
          if (n0 + nn < nout && (!KPAD || ka < KD)) v = MODE == 0 ? w[((size_t)(n0 + nn) * cin_total + ka) * TAPS + tap] : w[((size_t)ka * cin_total + n0 + nn) * TAPS + tap];
        } else {   // 1x1 dgrad: W[co = k][ci = n], coalesced along n
          const int kk = i / (32 * NT), nn = i - kk * (32 * NT);
          if (n0 + nn < nout) v = w[(size_t)kk * cin_total + n0 + nn];
        }
        t[j] = v;
      }
#pragma unroll
      for (int j = 0; j < WCH; ++j) {
        const int i = tid + 256 * (j0 + j);
        if (MODE == 0 || TAPS > 1) {
          const int nn = i / KW, kk = i - nn * KW;
          Ws[nn * LDA + kk] = t[j];
        } else {
          const int kk = i / (32 * NT), nn = i - kk * (32 * NT);
          Ws[nn * LDA + kk] = t[j];
        }
      }
    }
  };
  auto commit = [&](int tap) __attribute__((always_inline)) {
    const int kh = TAPS == 1 ? 1 : tap / 3, kw = TAPS == 1 ? 1 : tap - (tap / 3) * 3;
    const f4 one = (f4){1.f, 1.f, 1.f, 1.f}, zero = (f4){0.f, 0.f, 0.f, 0.f};
    if (MODE == 1 && PLAIN) {
#pragma unroll
      for (int p = 0; p < PF; ++p) *reinterpret_cast<f4*>(As + (row0 + p * RP) * LDA + 4 * c4) = pv[p] ? pa[p] : zero;
      return;
    }
    const float* gptr = av.gate;
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      int n = 0;
      if (gptr) n = LIN ? min(cur_tile * BM + row0 + p * RP, M - 1) / OHW : (rn[p] < 0 ? 0 : rn[p]);
      const f4 gate = gptr ? *reinterpret_cast<const f4*>(gptr + (size_t)n * av.cstride + cabs) : one;
      f4 v;
      if (MODE == 0) v = lhn_apply_xf(pa[p], xf) * gate;
      else v = lhn_dy_fast(xf, gr, pa[p], pb[(MODE == 1 && !PLAIN) ? p : 0], gate);
      *reinterpret_cast<f4*>(As + (row0 + p * RP) * LDA + 4 * c4) = pv[p] ? v : zero;
    }
  };

  int tile = blockIdx.x;
  if (tile < ntiles) {
    geom(tile);
    issue(tap_of(0), 0);
    stage_w(tap_of(0), 0);
    commit(tap_of(0));
  }
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    f16v acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const int next_tile = tile + gridDim.x;
    const int nph = ntaps * NSL;              // phases of a tile: (tap, K slice), slices innermost
    for (int q = 0; q < nph; ++q) {
      const bool more = (q + 1 < nph) || (next_tile < ntiles);
      const int qn = q + 1 < nph ? q + 1 : 0;
      const int ntap = tap_of(qn / NSL), nsl = NSL > 1 ? qn % NSL : 0;
      if (q + 1 < nph) issue(ntap, nsl);
      else if (next_tile < ntiles) {
        geom(next_tile);
        issue(ntap, nsl);
      }
      const float* arow = As + (wave * 32 + l31) * LDA + 4 * lh;
      const float* brow = Ws + l31 * LDA + 4 * lh;
#pragma unroll 4
      for (int kc = 0; kc < (KPAD && NSL == 1 ? (KD + 7) / 8 : KW / 8); ++kc) {
        const f4 a = *reinterpret_cast<const f4*>(arow + kc * 8);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const f4 b = *reinterpret_cast<const f4*>(brow + j * 32 * LDA + kc * 8);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[j], 0, 0, 0);
        }
      }
      if (more) {
        __syncthreads();                 // every wave is done reading this phase's LDS images
        if (TAPS > 1) stage_w(ntap, nsl);
        commit(ntap);
        __syncthreads();
      }
    }
    // ---- epilogue (C/D layout: col = lane&31 -> feature, row = (r&3) + 8*(r>>2) + 4*(lane>>5) -> pixel)
    const int mbase = tile * BM + wave * 32 + 4 * lh;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int ch = n0 + j * 32 + l31;
      if (ch >= nout) continue;
      TileStat ts;
      ts.reset();
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mbase + (r & 3) + 8 * (r >> 2);
        if (m < M) {
          const float v = acc[j][r];
          if (MODE == 0) {
            y.data[(size_t)m * y.cstride + y.coff + ch] = v;
            ts.add(v);
          } else {
            size_t pix = (size_t)m;
            if (par) {
              const int n = m / OHW, rr = m - n * OHW, i2 = rr / OW, j2 = rr - i2 * OW;
              pix = ((size_t)n * x.H + 2 * i2 + ph) * x.W + 2 * j2 + pw2;
            }
            float* o = dx + pix * x.cstride + x.coff + ch;
            *o = dx_acc ? *o + v : v;
          }
        }
      }
      if (MODE == 0) ts.flush(ssum[j], ssq[j]);
    }
  }
  if (MODE == 0 && stats) {
    __syncthreads();
    double* redd = reinterpret_cast<double*>(As);        // [4][32*NT][2] doubles inside the (now idle) A tile
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const double s = ssum[j] + __shfl_xor(ssum[j], 32, 64);
      const double q = ssq[j] + __shfl_xor(ssq[j], 32, 64);
      if (lh == 0) {
        redd[(wave * 32 * NT + j * 32 + l31) * 2 + 0] = s;
        redd[(wave * 32 * NT + j * 32 + l31) * 2 + 1] = q;
      }
    }
    __syncthreads();
    if (tid < 32 * NT && n0 + tid < nout) {
      double s = 0, q = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        s += redd[(k * 32 * NT + tid) * 2 + 0];
        q += redd[(k * 32 * NT + tid) * 2 + 1];
      }
      double* st = stats + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * nout;
      atomicAdd(st + n0 + tid, s);
      atomicAdd(st + nout + n0 + tid, q);
    }
    if (fin.counter && lhn_last_block(fin.counter)) lhn_bn_finalize_block(fin, stats);
  }
}

// wgrad: blockIdx.y = tap, blockIdx.z = group of 32*NTO output channels (co0).  When gridDim.x <= nrep every (pixel
// chunk, tap, co group) owns a private slice of gradient replica blockIdx.x and the flush is a plain read-add-write: the
// float atomics of the flush (gridDim.x * |dW| of them, ~38 G/s) were the whole cost of this kernel on small maps.
// wgrad: blockIdx.y = tap.  64-pixel tiles; dYs[m][co], Xs[m][ci] (X shifted by the tap) -> dW_tap += dY^T X.
template <int CIN, int NTO, int TAPS, bool PLAIN = false>
__global__ void __launch_bounds__(256) k_kxk_wgrad(lhn_view x, lhn_view y, lhn_gradview gy, float* __restrict__ dw, int stride,
                                                   int cout, int M, int ntiles, int nrep, int64_t rep_stride, int wstride) {
  // CIN = 40: the 64-channel X image with channels [40, 64) zero (kxk_kp); their columns of dW are never flushed
  constexpr int CINP = kxk_kp(CIN), NTI = CINP / 32, COP = 32 * NTO, LDY = COP + 4, LDX = CINP + 4;
  constexpr bool XPAD = CINP != CIN;
  // fewer dW tiles than waves (32 -> 32: one tile): split the 64-pixel K range of a tile over the idle waves; the partial
  // tiles meet in LDS before the flush
  constexpr int T = NTO * NTI, KS = T < 4 ? 4 / T : 1;
  constexpr int NDW = (T * KS + 3) / 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dYs = smem;               // [64][LDY]
  float* Xs = dYs + 64 * LDY;      // [64][LDX]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int tap = blockIdx.y, kh = TAPS == 1 ? 1 : tap / 3, kw = TAPS == 1 ? 1 : tap - (tap / 3) * 3;
  constexpr int XC4 = CINP / 4, XRP = 256 / XC4, XPF = 64 / XRP;
  constexpr int YC4 = COP / 4, YRP = 256 / YC4, YPF = 64 / YRP;
  const int xc4 = tid % XC4, xr0 = tid / XC4;
  const bool xcok = !XPAD || 4 * xc4 < CIN;
  const int xabs = x.coff + (xcok ? 4 * xc4 : 0);
  const int co0 = blockIdx.z * COP;
  const int yc4 = tid % YC4, yr0 = tid / YC4, yabs = y.coff + co0 + 4 * yc4;
  const Xf4 xxf = lhn_load_xf(x, xabs);
  const bool ych_ok = co0 + 4 * yc4 < cout;
  const Xf4 yxf = lhn_load_xf(y, ych_ok ? yabs : y.coff);
  const Gr4 ygr = lhn_load_coef(gy, y.cstride, ych_ok ? yabs : y.coff);
  const int HoWo = y.H * y.W;
  f16v accw[NDW];
#pragma unroll
  for (int t = 0; t < NDW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) accw[t][r] = 0.f;

  const f4 one = (f4){1.f, 1.f, 1.f, 1.f}, zero = (f4){0.f, 0.f, 0.f, 0.f};
  f4 xraw[XPF], yraw[PLAIN ? 1 : YPF], ydz[YPF];
  bool xok[XPF], yok[YPF];
  int xn[XPF], yn[YPF];
  // raw global loads of one 64-pixel tile into registers (clamped addresses, validity kept as predicates)
  auto issue = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < XPF; ++p) {
      const int m = min(tile * 64 + xr0 + p * XRP, M - 1);
      const int n = m / HoWo, r = m - n * HoWo, ho = r / y.W, wo = r - ho * y.W;
      const int ih = ho * stride - 1 + kh, iw = wo * stride - 1 + kw;
      const int ihc = min(max(ih, 0), x.H - 1), iwc = min(max(iw, 0), x.W - 1);
      xok[p] = xcok && (tile * 64 + xr0 + p * XRP < M) && ih == ihc && iw == iwc;
      xn[p] = n;
      xraw[p] = *reinterpret_cast<const f4*>(x.data + ((size_t)(n * x.H + ihc) * x.W + iwc) * x.cstride + xabs);
    }
#pragma unroll
    for (int p = 0; p < YPF; ++p) {
      const int m = min(tile * 64 + yr0 + p * YRP, M - 1);
      yok[p] = (tile * 64 + yr0 + p * YRP < M) && ych_ok;
      yn[p] = m / HoWo;
      const size_t off = (size_t)m * y.cstride + (ych_ok ? yabs : y.coff);
      if (!PLAIN) yraw[PLAIN ? 0 : p] = *reinterpret_cast<const f4*>(y.data + off);
      ydz[p] = *reinterpret_cast<const f4*>(gy.dz + off);
    }
  };
  // transform and park them in LDS
  auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < XPF; ++p) {
      const f4 gate = x.gate ? *reinterpret_cast<const f4*>(x.gate + (size_t)xn[p] * x.cstride + xabs) : one;
      const f4 v = lhn_apply_xf(xraw[p], xxf) * gate;
      *reinterpret_cast<f4*>(Xs + (xr0 + p * XRP) * LDX + 4 * xc4) = xok[p] ? v : zero;
    }
    if (PLAIN) {
#pragma unroll
      for (int p = 0; p < YPF; ++p) *reinterpret_cast<f4*>(dYs + (yr0 + p * YRP) * LDY + 4 * yc4) = yok[p] ? ydz[p] : zero;
    } else {
#pragma unroll
      for (int p = 0; p < YPF; ++p) {
        const f4 gate = (y.gate && ych_ok) ? *reinterpret_cast<const f4*>(y.gate + (size_t)yn[p] * y.cstride + yabs) : one;
        const f4 v = lhn_dy_fast(yxf, ygr, yraw[PLAIN ? 0 : p], ydz[p], gate);
        *reinterpret_cast<f4*>(dYs + (yr0 + p * YRP) * LDY + 4 * yc4) = yok[p] ? v : zero;
      }
    }
  };
  // The next tile's raw loads are issued before this tile's MFMA phase and parked in LDS after it (PF).  Only where every
  // wave owns whole dW tiles: the K-split instances (NTO*NTI < 4) produced wrong dW in this form on hipcc 7.2 and keep the
  // plain issue -> commit -> multiply order.
  constexpr bool PF = (KS == 1);
  int tile = blockIdx.x;
  if (PF && tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    if (!PF) issue(tile);
    commit();
    __syncthreads();
    if (PF && tile + (int)gridDim.x < ntiles) issue(tile + gridDim.x);
    if constexpr (KS == 1 && T % 4 == 0 && 4 % NTI == 0) {
      // whole tiles per wave: NO predicate around the MFMAs and the wave index in a scalar register.  With `if (tl < T)` in this
      // loop the compiler emitted exec-mask branches and an lgkmcnt(0) wait in front of every MFMA group: 128 -> 128 3x3 at
      // 64 x 64 took 840 us (58 % of the fp32 MFMA peak); this form: hourglass step 66.4 -> 64.3 ms, A 19.87 -> 19.39.  (A variant
      // with the three taps of a kernel row per workgroup -- one dY tile, a 66-pixel X run, 12 accumulator tiles per wave, one
      // workgroup per CU -- was built on top and measured 0.1-1 % SLOWER than one tap per workgroup: removed.)
      const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
      const float* ap = dYs + lh * LDY + l31 + 32 * (wv / NTI);
      const float* bp = Xs + lh * LDX + l31 + 32 * (wv % NTI);
#pragma unroll 4
      for (int ks = 0; ks < 32; ++ks) {
        const float b = bp[(2 * ks) * LDX];
        float a[NDW];
#pragma unroll
        for (int t = 0; t < NDW; ++t) a[t] = ap[(2 * ks) * LDY + 32 * (4 / NTI) * t];
#pragma unroll
        for (int t = 0; t < NDW; ++t) accw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b, accw[t], 0, 0, 0);
      }
    } else {
      const int kpart = KS > 1 ? wave % KS : 0;
#pragma unroll 4
      for (int ks = kpart * (32 / KS); ks < (kpart + 1) * (32 / KS); ++ks) {
        const float* dyr = dYs + (2 * ks + lh) * LDY + l31;
        const float* xr = Xs + (2 * ks + lh) * LDX + l31;
#pragma unroll
        for (int t = 0; t < NDW; ++t) {
          const int tl = (wave + 4 * t) / KS;
          if (tl < T) {
            const int it = tl / NTI, jt = tl % NTI;
            accw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(dyr[32 * it], xr[32 * jt], accw[t], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  const bool exclusive = (int)gridDim.x <= nrep;
  dw += (size_t)(blockIdx.x % nrep) * rep_stride;
  if (KS > 1) {
    // K-split: NDW == 1; waves of a tile (wave / KS equal) add their partials through LDS (dYs/Xs are dead), the first
    // wave of each tile keeps the sum
    float* part = dYs;                        // [4 waves][16 regs][64 lanes]
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(wave * 16 + r) * 64 + lane] = accw[0][r];
    __syncthreads();
    if (wave % KS == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < KS; ++k) v += part[((wave + k) * 16 + r) * 64 + lane];
        accw[0][r] = v;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NDW; ++t) {
    const int tl = (wave + 4 * t) / KS;
    if (tl < T && (KS == 1 || wave % KS == 0)) {
      const int it = tl / NTI, jt = tl % NTI;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + 32 * it + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (co < cout && (!XPAD || 32 * jt + l31 < CIN)) {
          float* o = dw + ((size_t)co * wstride + 32 * jt + l31) * TAPS + tap;     // wstride = input channels of the WHOLE weight
          if (exclusive) *o += accw[t][r];
          else atomicAdd(o, accw[t][r]);
        }
      }
    }
  }
}

// wt[tap][r][k]: mode 0 (forward GEMM, rows = Cout, K = Cin)  wt = w[r][k][tap];  mode 1 (dgrad, rows = Cin, K = Cout)
// wt = w[k][r][tap].  147,456 floats for 128 -> 128: a ~3 us launch per conv and direction.
__global__ void __launch_bounds__(256) k_w_tapmajor(const float* __restrict__ w, float* __restrict__ wt, int Cout, int Cin, int mode) {
  const int R = mode ? Cin : Cout, K = mode ? Cout : Cin, total = 9 * R * K;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k = i % K, r = (i / K) % R, tap = i / (K * R);
    wt[i] = mode ? w[((size_t)k * Cin + r) * 9 + tap] : w[((size_t)r * Cin + k) * 9 + tap];
  }
}
static void launch_w_tapmajor(const float* w, float* wt, int Cout, int Cin, int mode, hipStream_t s) {
  const int total = 9 * Cout * Cin;
  hipLaunchKernelGGL(k_w_tapmajor, dim3((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024), dim3(256), 0, s, w, wt, Cout, Cin, mode);
}

template <int KD, int NT, int MODE, int TAPS, bool PLAIN = false>
static int launch_kxk(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, double* stats, float* dx,
                      int dx_acc, int stride, int nout, hipStream_t s, const lhn_bnfin* finp = nullptr, int nsplit = 1, int parity = 0,
                      const float* wt = nullptr) {
  lhn_bnfin fin;
  if (finp && stats) fin = *finp; else fin.counter = nullptr;
  const lhn_view* ov = MODE == 0 ? y : x;
  const int M = parity ? ov->N * ((ov->H + 1) / 2) * ((ov->W + 1) / 2) : ov->N * ov->H * ov->W, ntiles = (M + 127) / 128;
  constexpr int KW = kxk_kw(KD);                // the K slice that is resident in LDS
  const size_t lds = (size_t)((32 * NT + 128) * (KW + 4) + 4 * 32 * NT * 2) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_kxk<KD, NT, MODE, TAPS, PLAIN>, lds, 4, &per_cu)) {
    lhn_set_error("lhn_conv_kxk: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  int grid = lhn_num_cus() * per_cu;
  if (grid > ntiles) grid = ntiles;
  lhn_gradview g;
  if (gy) g = *gy; else g.dz = g.dpool = g.coef = nullptr;
  hipLaunchKernelGGL((k_kxk<KD, NT, MODE, TAPS, PLAIN>), dim3(grid, nsplit, parity ? 4 : 1), dim3(256), lds, s, *x, w, *y, g, stats, dx, dx_acc, stride, nout, M, ntiles, fin, wt);
  return 0;
}

// gridDim.x of the nine-tap wgrad (x 9 taps x cosplit groups): a quarter of the CUs, or one pixel chunk per gradient replica --
// exclusive replica slices, no atomics in the flush (chunked = false: Cout = 256 is split over gridDim.z on long maps as well)
static int kxk_wgrad_grid(int cus, int ntiles, int nrep, int cosplit, bool chunked) {
  int grid = (cosplit > 1 && nrep > 1 && chunked) ? nrep : cus / 4;
  if (grid < 1) grid = 1;
  return grid > ntiles ? ntiles : grid;
}

template <int CIN, int NTO, int TAPS, bool PLAIN = false>
static int launch_kxk_wgrad(const lhn_view* x, const lhn_view* y, const lhn_gradview* gy, float* dw, int stride, int nrep,
                            int64_t rep_stride, hipStream_t s, int cosplit = 1, int wstride = CIN, bool chunked = true) {
  const int M = y->N * y->H * y->W, ntiles = (M + 63) / 64;
  constexpr int COP = 32 * NTO;
  const size_t lds = (size_t)(64 * (COP + 4) + 64 * (kxk_kp(CIN) + 4)) * sizeof(float);
  static LhnKernelCfg cfg;
  int per_cu = 1;
  if (!lhn_kernel_cfg(cfg, &k_kxk_wgrad<CIN, NTO, TAPS, PLAIN>, lds, 3, &per_cu)) {
    lhn_set_error("lhn_conv_kxk_bwd: cannot reserve %zu B of LDS", lds);
    return 2;
  }
  int grid = TAPS == 1 ? lhn_num_cus() * per_cu / cosplit : kxk_wgrad_grid(lhn_num_cus(), ntiles, nrep, cosplit, chunked);
  if (grid < 1) grid = 1;
  if (grid > ntiles) grid = ntiles;
  hipLaunchKernelGGL((k_kxk_wgrad<CIN, NTO, TAPS, PLAIN>), dim3(grid, TAPS, cosplit), dim3(256), lds, s, *x, *y, *gy, dw, stride, y->C, M, ntiles, nrep,
                     rep_stride, wstride);
  return 0;
}

// =====================================================================================================
// Instances: one list per kernel template.  The launch switches and kxk_name() (the printed name; NULL = no instance) are generated
// from them and nothing else states the set.  K = 32, 64 or 128 channels exactly, 1, 2 or 4 tiles of 32 per block; K = 256 is two
// 128-channel slices: inside k_kxk (forward and plain dgrad only), and one k_kxk_wgrad<128, ...> launch per slice.  The one-tap
// pairs are those of lhn_pw_bwd_split (LHN_KXK_ONETAP, lhn_common.h).
// Width 160 (kxk_pair_ok: 160 -> 160 and 40 -> 40 only): K = 160 is five 32-channel slices inside k_kxk with five feature tiles in
// one block or one per block (forward and plain dgrad), K = 40 the padded 64-channel image with one or two tiles; the weight
// gradient of a 160-channel x is a k_kxk_wgrad<128, ...> launch and a <32, ...> launch, of a 40-channel x one <40, 2, ...>.
#define KXK_NT(X, K, ...) X(K, 1, __VA_ARGS__) X(K, 2, __VA_ARGS__) X(K, 4, __VA_ARGS__)
#define KXK_NT40(X, ...) X(40, 1, __VA_ARGS__) X(40, 2, __VA_ARGS__)
#define KXK_NT160(X, ...) X(160, 1, __VA_ARGS__) X(160, 5, __VA_ARGS__)
// k_kxk<KD, NT, MODE, TAPS, PLAIN>: forward; dgrad of the in-place dy; dgrad with dy on the fly; one tap
#define KXK_INSTANCES(X)                                                                                                \
  KXK_NT(X, 32, 0, 9, false) KXK_NT(X, 64, 0, 9, false) KXK_NT(X, 128, 0, 9, false) KXK_NT(X, 256, 0, 9, false)         \
  KXK_NT(X, 32, 1, 9, true) KXK_NT(X, 64, 1, 9, true) KXK_NT(X, 128, 1, 9, true) KXK_NT(X, 256, 1, 9, true)             \
  KXK_NT(X, 32, 1, 9, false) KXK_NT(X, 64, 1, 9, false) KXK_NT(X, 128, 1, 9, false) LHN_KXK_ONETAP(X, 1, 1, true)       \
  KXK_NT40(X, 0, 9, false) KXK_NT40(X, 1, 9, true) KXK_NT40(X, 1, 9, false) KXK_NT160(X, 0, 9, false) KXK_NT160(X, 1, 9, true)
// k_kxk_wgrad<CIN, NTO, TAPS, PLAIN>
#define KXK_WGRAD_INSTANCES(X)                                                                                          \
  KXK_NT(X, 32, 9, true) KXK_NT(X, 64, 9, true) KXK_NT(X, 128, 9, true) KXK_NT(X, 32, 9, false) KXK_NT(X, 64, 9, false) \
  KXK_NT(X, 128, 9, false) LHN_KXK_ONETAP(X, 1, true) X(40, 2, 9, true) X(40, 2, 9, false)

constexpr int KXK_WGRAD = 2;      // KxkInst::mode of a k_kxk_wgrad instance (0 forward, 1 dgrad: k_kxk's MODE)
struct KxkInst {
  int k, nt, mode, taps;          // k = 0: none
  bool plain;
};
constexpr int kxk_key(int k, int nt, int mode, int taps, bool plain) { return (((k * 8 + nt) * 4 + mode) * 16 + taps) * 2 + (plain ? 1 : 0); }
constexpr int kxk_key(const KxkInst& i) { return kxk_key(i.k, i.nt, i.mode, i.taps, i.plain); }

static const char* kxk_name(const KxkInst& i) {
  switch (kxk_key(i)) {
#define X(K, NT, MODE, TAPS, PLAIN) case kxk_key(K, NT, MODE, TAPS, PLAIN): return "k_kxk<" #K ", " #NT ", " #MODE ", " #TAPS ", " #PLAIN ">";
    KXK_INSTANCES(X)
#undef X
#define X(K, NT, TAPS, PLAIN) case kxk_key(K, NT, KXK_WGRAD, TAPS, PLAIN): return "k_kxk_wgrad<" #K ", " #NT ", " #TAPS ", " #PLAIN ">";
    KXK_WGRAD_INSTANCES(X)
#undef X
  }
  return nullptr;
}

static int kxk_launch(const KxkInst& i, const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, double* stats, float* dx,
                      int dx_acc, int stride, int nout, hipStream_t s, const lhn_bnfin* fin, int nsplit, int parity, const float* wt) {
  switch (kxk_key(i)) {
#define X(K, NT, MODE, TAPS, PLAIN) \
  case kxk_key(K, NT, MODE, TAPS, PLAIN): return launch_kxk<K, NT, MODE, TAPS, PLAIN>(x, w, y, gy, stats, dx, dx_acc, stride, nout, s, fin, nsplit, parity, wt);
    KXK_INSTANCES(X)
#undef X
  }
  LHN_CHECK_ARG(false, "lhn_conv_kxk: no k_kxk instance for K = %d, %d tiles", i.k, i.nt);
}

static int kxk_wgrad_launch(const KxkInst& i, const lhn_view* x, const lhn_view* y, const lhn_gradview* gy, float* dw, int stride, int nrep,
                            int64_t rep_stride, hipStream_t s, int cosplit, int wstride, bool chunked) {
  switch (kxk_key(i)) {
#define X(K, NT, TAPS, PLAIN) \
  case kxk_key(K, NT, KXK_WGRAD, TAPS, PLAIN): return launch_kxk_wgrad<K, NT, TAPS, PLAIN>(x, y, gy, dw, stride, nrep, rep_stride, s, cosplit, wstride, chunked);
    KXK_WGRAD_INSTANCES(X)
#undef X
  }
  LHN_CHECK_ARG(false, "lhn_conv_kxk: no k_kxk_wgrad instance for %d channels, %d tiles", i.k, i.nt);
}

// =====================================================================================================
// Route: which kernels a dense 3x3 call launches.  kxk_fwd_route() and kxk_bwd_route() are pure and the only place that knows the
// rules; the dispatchers below and lhn_conv_kxk_route() (the host-only query, which the tests and profiles/kxk_instances.md read)
// call them.  `cus` is what lhn_num_cus() reports: deterministic mode is cus = 2.
struct KxkShape {
  int N, H, W;                    // of x
  int Cin, Cout, stride, nrep;
  bool dx, dpool;                 // backward: dx wanted, a pooled gradient rides in gy
};
struct KxkRoute {
  bool ok;                        // false: no instance, the call is refused before any launch
  bool plain;                     // backward: k_dy_inplace in front (dz := dy), the kernels stream dy
  KxkInst conv;                   // the forward or the data gradient (k = 0: dx is NULL, no dgrad and none needed)
  int nsplit, par;                //   blocks of 32 * nt features on gridDim.y;  stride-2 dgrad: four pixel-parity classes on gridDim.z
  KxkInst wgrad;                  // backward: the weight gradient, one launch per slice of wgrad.k input channels
  KxkInst wtail;                  //   (Cin = 160: k = 32) one more launch for the channels past the last whole slice; k = 0: none
  int nslices, cosplit;           //   (Cin = 256: two);  groups of 32 * nt output channels on gridDim.z
  bool chunked, exclusive;        //   pixel chunks = gradient replicas;  the flush is a plain read-add-write (gridDim.x <= nrep)
};

// LHN_PLAIN, read from the environment on first use: 0 = unset (the size rule), else LHN_KXK_SW_PLAIN0 / LHN_KXK_SW_PLAIN1
static int kxk_switches() {
  static const int v = [] { const char* e = getenv("LHN_PLAIN"); return !e ? 0 : e[0] == '1' ? LHN_KXK_SW_PLAIN1 : LHN_KXK_SW_PLAIN0; }();
  return v;
}

static int kxk_out_pixels(const KxkShape& s) { return s.N * ((s.H - 1) / s.stride + 1) * ((s.W - 1) / s.stride + 1); }

// Small maps give few 128-pixel tiles (8x8 maps at batch 64: 32 tiles for 256 CUs): split the `nt` 32-feature tiles of the GEMM's N
// over gridDim.y so that about two workgroups per CU exist.  Returns the per-block tile count (1, 2 or 4 -> nt / splits blocks).
// nt = 8 (256 features) starts from two splits: a block holds at most four accumulator tiles.  0: not 1, 2, 4, 5 or 8 tiles.
// nt = 5 (160 features) has no halves: all five tiles in one block (the A tile is staged once) where that alone gives two workgroups
// per CU, else one tile per block on gridDim.y = 5.
static int kxk_nt_block(int M, int nt, int cus) {
  const int ntiles = (M + 127) / 128;
  if (nt == 5) return ntiles >= 2 * cus ? 5 : 1;
  if (nt > 8 || (nt & (nt - 1))) return 0;
  int splits = nt > 4 ? nt / 4 : 1;
  while (splits < nt && ntiles * splits < 2 * cus) splits *= 2;
  return nt / splits;
}

// Width 160 serves mynet's own convolutions: 160 -> 160 and 40 -> 40.  Every other pair with a side of 160, and every other pair that
// would need the padded K = 40 (Cin = 40; the data gradient of Cout = 40), is refused.  64 -> 40 and 256 -> 40 forward are older than
// this rule and need no K = 40: they stay.
static bool kxk_pair_ok(const KxkShape& s, bool backward) {
  // five feature tiles (kxk_nt_block, the weight gradient's groups) exist for 160 alone: 129 .. 159 channels stay refused
  if (((s.Cout + 31) / 32 == 5 && s.Cout != 160) || ((s.Cin + 31) / 32 == 5 && s.Cin != 160)) return false;
  if (s.Cin == 160 || s.Cout == 160 || s.Cin == 40) return s.Cin == s.Cout;
  return !(backward && s.dx && s.Cout == 40);
}

static KxkRoute kxk_fwd_route(const KxkShape& s, int cus, int) {
  KxkRoute r = {};
  if (!kxk_pair_ok(s, false)) return r;
  const int ntot = (s.Cout + 31) / 32, nt = kxk_nt_block(kxk_out_pixels(s), ntot, cus);      // GEMM N = Cout, K = Cin
  r.conv = {s.Cin, nt, 0, 9, false};
  r.nsplit = nt ? ntot / nt : 0;
  r.ok = kxk_name(r.conv) != nullptr;
  return r;
}

static KxkRoute kxk_bwd_route(const KxkShape& s, int cus, int sw) {
  KxkRoute r = {};
  if (!kxk_pair_ok(s, true)) return r;
  // Large channel counts: turn dz into dy in place, then stream it plain (LHN_PLAIN=0/1 overrides the size rule).  A channel-attention
  // pooled gradient always takes this path: lhn_dy_fast has no pooled term.  So does a side of 256 channels: the sliced dgrad has no
  // dy-on-the-fly instance (a second set of y-transform and coefficient registers per slice), and by the size rule it is plain anyway.
  r.plain = s.dpool || s.Cin > 128 || s.Cout > 128 ||
            ((sw & LHN_KXK_SW_PLAIN1) ? true : (sw & LHN_KXK_SW_PLAIN0) ? false : s.Cin * s.Cout >= 64 * 64);
  if (s.dx) {      // GEMM N = Cin, K = Cout (256: two slices inside the kernel, dx written once)
    const int ntot = (s.Cin + 31) / 32, nt = kxk_nt_block(s.N * s.H * s.W, ntot, cus);
    r.conv = {s.Cout, nt, 1, 9, r.plain};
    r.nsplit = nt ? ntot / nt : 0;
    r.par = s.stride == 2;
  }
  // Cout >= 64: one 32-channel group per block (gridDim.z), pixel chunks = gradient replicas -> atomic-free flush (only while a pixel
  // chunk stays short: <= 16 tiles of 64 pixels per block; big maps amortise the atomic flush).  Cout = 256: eight groups the same
  // way, or two groups of four tiles (a block holds at most four) with the atomic flush.
  const int wtot = (s.Cout + 31) / 32, wtiles = (kxk_out_pixels(s) + 63) / 64;
  r.chunked = s.Cin >= 64 && s.nrep > 1 && wtiles <= 16 * s.nrep;
  // Cout = 160: five groups of one tile the same way, or three groups of two tiles (the last group's second tile is past Cout: its
  // dy columns are zeros) with the atomic flush.
  r.cosplit = wtot == 8 ? (r.chunked ? 8 : 2) : wtot == 5 ? (r.chunked ? 5 : 3) : ((wtot == 2 || wtot == 4) && r.chunked ? wtot : 1);
  // Cin = 256: once per 128-channel input slice (disjoint columns of dW).  Cin = 160: a 128-channel slice and a 32-channel one.
  r.nslices = s.Cin == 256 ? 2 : 1;
  const int nto = (wtot + r.cosplit - 1) / r.cosplit;
  r.wgrad = {s.Cin == 160 ? 128 : s.Cin / r.nslices, nto, KXK_WGRAD, 9, r.plain};
  if (s.Cin == 160) r.wtail = {32, nto, KXK_WGRAD, 9, r.plain};
  r.exclusive = kxk_wgrad_grid(cus, wtiles, s.nrep, r.cosplit, r.chunked) <= s.nrep;
  r.ok = (!s.dx || kxk_name(r.conv)) && kxk_name(r.wgrad) && (!r.wtail.k || kxk_name(r.wtail)) && s.Cin % r.nslices == 0;
  return r;
}

// =====================================================================================================
// Dispatchers: validate, ask the route, refuse BEFORE the first launch (a refused call writes nothing, not even the weight scratch;
// k_dy_inplace consumes dz and the dgrad writes dx, so a call refused after them would leave both changed), launch.
static int kxk_geometry_ok(const lhn_view* x, const lhn_view* y, int stride) {
  return y->N == x->N && y->H == (x->H - 1) / stride + 1 && y->W == (x->W - 1) / stride + 1;
}

extern "C" int lhn_conv_kxk_fwd(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int stride,
                                const lhn_bnfin* fin, float* wt_scratch, void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && w && lhn_no_pend(x), "lhn_conv_kxk_fwd: bad view / null pointer (no pending BatchNorm here)");
  LHN_CHECK_ARG((stride == 1 || stride == 2) && kxk_geometry_ok(x, y, stride), "lhn_conv_kxk_fwd: geometry / stride %d", stride);
  const KxkRoute r = kxk_fwd_route({x->N, x->H, x->W, x->C, y->C, stride, 1, false, false}, lhn_num_cus(), kxk_switches());
  LHN_CHECK_ARG(r.ok, "lhn_conv_kxk_fwd: unsupported channels Cin=%d Cout=%d", x->C, y->C);
  hipStream_t s = (hipStream_t)stream;
  if (wt_scratch) launch_w_tapmajor(w, wt_scratch, y->C, x->C, 0, s);
  const int rc = kxk_launch(r.conv, x, w, y, nullptr, stats, nullptr, 0, stride, y->C, s, fin, r.nsplit, 0, wt_scratch);
  if (rc) return rc;
  LHN_CHECK_LAUNCH("lhn_conv_kxk_fwd");
  return 0;
}

extern "C" int lhn_conv_kxk_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                                int dx_accumulate, float* dw, int stride, int nrep, int64_t rep_stride, float* wt_scratch,
                                void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(x) && lhn_view_ok(y) && w && gy && gy->dz && dw && lhn_no_pend(x) && lhn_no_pend(y), "lhn_conv_kxk_bwd: bad view / null pointer");
  LHN_CHECK_ARG((stride == 1 || stride == 2) && kxk_geometry_ok(x, y, stride), "lhn_conv_kxk_bwd: geometry / stride %d", stride);
  if (nrep < 1) nrep = 1;
  const KxkRoute r = kxk_bwd_route({x->N, x->H, x->W, x->C, y->C, stride, nrep, dx != nullptr, gy->dpool != nullptr}, lhn_num_cus(), kxk_switches());
  LHN_CHECK_ARG(r.ok, "lhn_conv_kxk_bwd: unsupported channels Cin=%d Cout=%d", x->C, y->C);
  hipStream_t s = (hipStream_t)stream;
  if (r.plain) launch_dy_inplace(y, gy, s);
  if (r.conv.k) {
    if (wt_scratch) launch_w_tapmajor(w, wt_scratch, y->C, x->C, 1, s);
    const int rc = kxk_launch(r.conv, x, w, y, gy, nullptr, dx, dx_accumulate, stride, x->C, s, nullptr, r.nsplit, r.par, wt_scratch);
    if (rc) return rc;
  }
  for (int k0 = 0; k0 < x->C;) {      // row length of dW = Cin (wstride), the slice starts 9 * k0 in
    const KxkInst& wi = x->C - k0 >= r.wgrad.k ? r.wgrad : r.wtail;
    lhn_view xv = *x;
    xv.coff += k0;
    xv.C = wi.k;
    const int rc = kxk_wgrad_launch(wi, &xv, y, gy, dw + (size_t)9 * k0, stride, nrep, rep_stride, s, r.cosplit, x->C, r.chunked);
    if (rc) return rc;
    k0 += wi.k;
  }
  LHN_CHECK_LAUNCH("lhn_conv_kxk_bwd");
  return 0;
}

// Host only: the names of what the two dispatchers would launch, in order (include/lhn.h).
extern "C" const char* lhn_conv_kxk_route(int backward, int N, int H, int W, int Cin, int Cout, int stride, int nrep, int features, int cus,
                                          int switches) {
  if ((stride != 1 && stride != 2) || N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return nullptr;
  const KxkShape sh = {N, H, W, Cin, Cout, stride, nrep < 1 ? 1 : nrep, (features & LHN_KXK_F_DX) != 0, (features & LHN_KXK_F_DPOOL) != 0};
  const KxkRoute r = (backward ? kxk_bwd_route : kxk_fwd_route)(sh, cus > 0 ? cus : lhn_num_cus(), switches < 0 ? kxk_switches() : switches);
  if (!r.ok) return nullptr;
  static thread_local char buf[320];
  size_t len = 0;
  auto put = [&](const char* fmt, auto... a) { len += snprintf(buf + len, sizeof(buf) - len, fmt, a...); };      // (the longest answer is 163 characters)
  auto launch = [&](const char* name) { put(len ? " + %s" : "%s", name); };
  if (r.plain) launch("k_dy_inplace");
  if (r.conv.k) {
    if (features & LHN_KXK_F_WT) launch("k_w_tapmajor");
    launch(kxk_name(r.conv));
    if (r.nsplit > 1) put(" y%d", r.nsplit);
    if (r.par) put("%s", " par");
  }
  if (backward) {
    launch(kxk_name(r.wgrad));
    if (r.cosplit > 1) put(" z%d", r.cosplit);
    put(" %s", r.exclusive ? "excl" : "atomic");
    if (r.nslices > 1) put(" x %d", r.nslices);
    if (r.wtail.k) {
      launch(kxk_name(r.wtail));
      if (r.cosplit > 1) put(" z%d", r.cosplit);
      put(" %s", r.exclusive ? "excl" : "atomic");
    }
  }
  return buf;
}

// 1x1 backward as three launches (k_dy_inplace, dgrad, wgrad = the per-tap kernel with one tap): lhn_conv_pw_bwd takes it for large
// Cin*Cout where the fused kernel is LDS-bound to one block per CU.  Channel counts above 128 (hourglass: 256) run as 128-wide
// slices: dgrad accumulates over output-channel slices (its K), wgrad runs once per input-channel slice with the output channels
// on gridDim.z (lhn_pw_split_tiles, lhn_common.h).  pw_bwd_route (k_conv_pw.hip) has checked that every slice has an instance
// (lhn_pw_split_instance) and says which kernel the data gradient takes: dy is formed in place, so nothing can be refused from here on.
int lhn_pw_bwd_split(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, float* dbias, int nrep, int64_t rep_stride, int dgrad, hipStream_t s) {
  const int Cin = x->C, Cout = y->C;
  const LhnPwSplitTiles t = lhn_pw_split_tiles(Cin, Cout);
  launch_dy_inplace(y, gy, s, dbias, nrep, rep_stride);
  // K = 256 in one pass on the register-W kernel (dy as input, W transposed: no second K slice accumulating into dx), else <= 128
  const int cc = dgrad == LHN_PW_DGRAD_WR256 ? 256 : t.cc;
  for (int co0 = 0; dgrad != LHN_PW_DGRAD_NONE && co0 < Cout; co0 += cc) {
    lhn_view yv = *y;
    yv.coff += co0;
    yv.C = cc;
    const float* wv = w + (size_t)co0 * Cin;
    const int acc = dx_accumulate || co0 > 0;
    int rc = 0;
    if (dgrad == LHN_PW_DGRAD_KXK) {
      rc = kxk_launch({cc, t.ntd, 1, 1, true}, x, wv, &yv, gy, nullptr, dx, acc, 1, Cin, s, nullptr, t.nsplit, 0, nullptr);
    } else {      // the register-resident-weights 1x1 kernel (k_conv_pw.hip) run on dy with W transposed, <= 128 input channels per launch
      lhn_view dyv = yv, dxv = *x;
      dyv.data = const_cast<float*>(gy->dz);
      dxv.data = dx;
      dyv.table = dxv.table = nullptr;
      dyv.gate = dxv.gate = nullptr;
      dyv.pend = dxv.pend = nullptr;
      dxv.C = t.kc;
      for (int ci0 = 0; ci0 < Cin && !rc; ci0 += t.kc) {
        dxv.coff = x->coff + ci0;
        rc = lhn_pw_dgrad_wr(&dyv, wv + ci0, &dxv, Cin, acc, s);
      }
    }
    if (rc) return rc;
  }
  for (int k0 = 0; k0 < Cin; k0 += t.kc) {
    lhn_view xv = *x;
    xv.coff += k0;
    xv.C = t.kc;
    const int rc = kxk_wgrad_launch({t.kc, t.nto, KXK_WGRAD, 1, true}, &xv, y, gy, dw + k0, 1, nrep, rep_stride, s, t.cosplit, Cin, true);
    if (rc) return rc;
  }
  return 0;
}
