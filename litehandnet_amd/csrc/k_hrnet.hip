// Elementwise pieces that only the Lite-HRNet baseline needs (models/pose_estimation/lite_hrnet.py; BASELINE config 5):
//   channel shuffle of a two-way concatenation (:29-52,141-142,246-247), the product with a nearest-upsampled weight map
//   (:105-107) and its backward, and the backward of the bilinear (align_corners=True) upsample-add (:272-275).
// NHWC fp32, thread = (group of 4 destination channels, pixel lane), HBM-bound; the forward of the product / bilinear
// combine lives in k_ew_fwd (k_misc.hip: EwSrcs.mode).
#include "lhn_common.h"

static inline int grid_cap(int64_t blocks, int cap_per_cu) {
  const int64_t cap = (int64_t)lhn_num_cus() * cap_per_cu;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// consumed value of 2 consecutive channels (absolute index c, even) at a pixel
struct Xf2 {
  float sc[2], sh[2], sl[2];
};
__device__ __forceinline__ Xf2 load_xf2(const lhn_view& v, int c) {
  Xf2 t;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    t.sc[j] = v.table ? v.table[c + j] : 1.f;
    t.sh[j] = v.table ? v.table[v.cstride + c + j] : 0.f;
    t.sl[j] = v.table ? v.table[2 * v.cstride + c + j] : 1.f;
  }
  return t;
}

// ------------------------------------------------------------------ channel_shuffle(cat(a, b), groups = 2)
// dst channel 2j = a[j], 2j+1 = b[j]; dst is stored plain (table identity).  One thread writes 4 dst channels =
// a[2g], b[2g], a[2g+1], b[2g+1].
__global__ void __launch_bounds__(256) k_shuffle2_fwd(lhn_view a, lhn_view b, lhn_view dst) {
  const int C4 = dst.C >> 2, c4 = threadIdx.x % C4, pl = threadIdx.x / C4, PL = 256 / C4;
  const int ca = a.coff + 2 * c4, cb = b.coff + 2 * c4;
  const Xf2 xa = load_xf2(a, ca), xb = load_xf2(b, cb);
  const int rows = dst.N * dst.H;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int n = row / dst.H;
    float ga[2] = {1.f, 1.f}, gb[2] = {1.f, 1.f};
    if (a.gate) { ga[0] = a.gate[(size_t)n * a.cstride + ca]; ga[1] = a.gate[(size_t)n * a.cstride + ca + 1]; }
    if (b.gate) { gb[0] = b.gate[(size_t)n * b.cstride + cb]; gb[1] = b.gate[(size_t)n * b.cstride + cb + 1]; }
    for (int w = LHN_LANE0(pl, PL); w < dst.W; w += PL) {
      const size_t pix = (size_t)row * dst.W + w;
      const float2 ra = *reinterpret_cast<const float2*>(a.data + pix * a.cstride + ca);
      const float2 rb = *reinterpret_cast<const float2*>(b.data + pix * b.cstride + cb);
      f4 o;
      o.x = lhn_lrelu(ra.x * xa.sc[0] + xa.sh[0], xa.sl[0]) * ga[0];
      o.y = lhn_lrelu(rb.x * xb.sc[0] + xb.sh[0], xb.sl[0]) * gb[0];
      o.z = lhn_lrelu(ra.y * xa.sc[1] + xa.sh[1], xa.sl[1]) * ga[1];
      o.w = lhn_lrelu(rb.y * xb.sc[1] + xb.sh[1], xb.sl[1]) * gb[1];
      *reinterpret_cast<f4*>(dst.data + pix * dst.cstride + dst.coff + 4 * c4) = o;
    }
  }
}
// d(value of a)[j] (+)= d(dst)[2j], d(value of b)[j] (+)= d(dst)[2j+1]   (da / db: gradient buffers with a's / b's geometry)
__global__ void __launch_bounds__(256) k_shuffle2_bwd(lhn_view a, lhn_view b, lhn_view dst, const float* __restrict__ ddst,
                                                      float* __restrict__ da, int acc_a, float* __restrict__ db, int acc_b) {
  const int C4 = dst.C >> 2, c4 = threadIdx.x % C4, pl = threadIdx.x / C4, PL = 256 / C4;
  const int ca = a.coff + 2 * c4, cb = b.coff + 2 * c4;
  const int rows = dst.N * dst.H;
  for (int row = blockIdx.x; row < rows; row += gridDim.x)
    for (int w = LHN_LANE0(pl, PL); w < dst.W; w += PL) {
      const size_t pix = (size_t)row * dst.W + w;
      const f4 g = *reinterpret_cast<const f4*>(ddst + pix * dst.cstride + dst.coff + 4 * c4);
      if (da) {
        float2* o = reinterpret_cast<float2*>(da + pix * a.cstride + ca);
        float2 v = make_float2(g.x, g.z);
        if (acc_a) { v.x += o->x; v.y += o->y; }
        *o = v;
      }
      if (db) {
        float2* o = reinterpret_cast<float2*>(db + pix * b.cstride + cb);
        float2 v = make_float2(g.y, g.w);
        if (acc_b) { v.x += o->x; v.y += o->y; }
        *o = v;
      }
    }
}

// ------------------------------------------------------------------ backward of dst = value(a) * up_nearest(value(g))
// One launch per operand, gather form (every source element sums the destination elements that read it):
//   d(src)[p] (+)= sum_{q reads p} d(dst)[q] * value(other at q)
__device__ __forceinline__ int nearest_src2(int d, int in, int out) {
  if (in == out) return d;
  const float sc = (float)in / (float)out;
  const int s = (int)floorf((float)d * sc);
  return s < in - 1 ? s : in - 1;
}
__global__ void __launch_bounds__(256) k_ew_mul_bwd(lhn_view src, lhn_view other, lhn_view dst, const float* __restrict__ ddst,
                                                    float* __restrict__ dsrc, int accumulate) {
  const int C4 = src.C >> 2, c4 = threadIdx.x % C4, pl = threadIdx.x / C4, PL = 256 / C4;
  const int fh = dst.H / src.H, fw = dst.W / src.W;        // integer fan-out (host-checked)
  const int cs = src.coff + 4 * c4, co = other.coff + 4 * c4, cd = dst.coff + 4 * c4;
  const Xf4 oxf = lhn_load_xf(other, co);
  const int rows = src.N * src.H;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int n = row / src.H, h = row - n * src.H;
    const f4 og = other.gate ? *reinterpret_cast<const f4*>(other.gate + (size_t)n * other.cstride + co) : (f4){1.f, 1.f, 1.f, 1.f};
    for (int w = LHN_LANE0(pl, PL); w < src.W; w += PL) {
      f4 g = (f4){0.f, 0.f, 0.f, 0.f};
      for (int a = 0; a < fh; ++a)
        for (int b = 0; b < fw; ++b) {
          const int hd = h * fh + a, wd = w * fw + b;
          const int ho = nearest_src2(hd, other.H, dst.H), wo = nearest_src2(wd, other.W, dst.W);
          const f4 ov = lhn_apply_xf(*reinterpret_cast<const f4*>(other.data + ((size_t)(n * other.H + ho) * other.W + wo) * other.cstride + co), oxf) * og;
          g += *reinterpret_cast<const f4*>(ddst + ((size_t)(n * dst.H + hd) * dst.W + wd) * dst.cstride + cd) * ov;
        }
      float* o = dsrc + ((size_t)row * src.W + w) * src.cstride + cs;
      if (accumulate) g += *reinterpret_cast<const f4*>(o);
      *reinterpret_cast<f4*>(o) = g;
    }
  }
}

// ------------------------------------------------------------------ backward of the bilinear (align_corners) source of a combine
// d(src)[hs, ws] (+)= sum over destination pixels whose taps include (hs, ws) of d(dst) * weight   (gather form)
__device__ __forceinline__ void bil_taps2(int d, int in, int out, int& i0, int& i1, float& w1) {
  if (in == out || out == 1) {
    i0 = i1 = (in == out) ? d : 0;
    w1 = 0.f;
    return;
  }
  const float pos = (float)d * ((float)(in - 1) / (float)(out - 1));
  i0 = (int)floorf(pos);
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  w1 = pos - (float)i0;
}
__global__ void __launch_bounds__(256) k_bilinear_bwd(lhn_view src, lhn_view dst, const float* __restrict__ ddst,
                                                      float* __restrict__ dsrc, int accumulate, float out_slope) {
  const int C4 = src.C >> 2, c4 = threadIdx.x % C4, pl = threadIdx.x / C4, PL = 256 / C4;
  const int cs = src.coff + 4 * c4, cd = dst.coff + 4 * c4;
  // destination indices that can touch source index i: d in [ (i-1)*(out-1)/(in-1), (i+1)*(out-1)/(in-1) ] (conservative +-1)
  const float rh = src.H > 1 ? (float)(dst.H - 1) / (float)(src.H - 1) : 0.f, rw = src.W > 1 ? (float)(dst.W - 1) / (float)(src.W - 1) : 0.f;
  const int rows = src.N * src.H;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const int n = row / src.H, h = row - n * src.H;
    const int hd0 = src.H > 1 ? max(0, (int)floorf((float)(h - 1) * rh) - 1) : 0;
    const int hd1 = src.H > 1 ? min(dst.H - 1, (int)ceilf((float)(h + 1) * rh) + 1) : dst.H - 1;
    for (int w = LHN_LANE0(pl, PL); w < src.W; w += PL) {
      const int wd0 = src.W > 1 ? max(0, (int)floorf((float)(w - 1) * rw) - 1) : 0;
      const int wd1 = src.W > 1 ? min(dst.W - 1, (int)ceilf((float)(w + 1) * rw) + 1) : dst.W - 1;
      f4 g = (f4){0.f, 0.f, 0.f, 0.f};
      for (int hd = hd0; hd <= hd1; ++hd) {
        int a0, a1;
        float ah;
        bil_taps2(hd, src.H, dst.H, a0, a1, ah);
        const float wh = (a0 == h ? 1.f - ah : 0.f) + (a1 == h ? ah : 0.f);
        if (wh == 0.f) continue;
        for (int wd = wd0; wd <= wd1; ++wd) {
          int b0, b1;
          float aw;
          bil_taps2(wd, src.W, dst.W, b0, b1, aw);
          const float ww = (b0 == w ? 1.f - aw : 0.f) + (b1 == w ? aw : 0.f);
          if (ww == 0.f) continue;
          const size_t pd = ((size_t)(n * dst.H + hd) * dst.W + wd) * dst.cstride + cd;
          f4 e = *reinterpret_cast<const f4*>(ddst + pd);
          if (out_slope != 1.f) {
            const f4 o = *reinterpret_cast<const f4*>(dst.data + pd);
            e.x *= o.x > 0.f ? 1.f : out_slope;
            e.y *= o.y > 0.f ? 1.f : out_slope;
            e.z *= o.z > 0.f ? 1.f : out_slope;
            e.w *= o.w > 0.f ? 1.f : out_slope;
          }
          g += e * (wh * ww);
        }
      }
      float* o = dsrc + ((size_t)row * src.W + w) * src.cstride + cs;
      if (accumulate) g += *reinterpret_cast<const f4*>(o);
      *reinterpret_cast<f4*>(o) = g;
    }
  }
}

// ------------------------------------------------------------------ ConditionalChannelWeighting as four grouped launches (inference)
// lite_hrnet.py:76-143 without train-mode BatchNorm is four dependent steps -- pool, gate, convolve, gate again and shuffle -- and each
// kernel below serves ALL 2..4 branches of a block in one grid: the workgroups of the small branches run beside those of the large
// ones instead of in launches of their own (the maps are 64^2 .. 8^2 at a 256^2 image: the family is launch-bound).
// A workgroup finds its branch from blockIdx.x against per-branch block offsets (scalar: the branch's views come out of the kernel
// arguments with scalar loads).  No atomics anywhere: sums are taken in a fixed order.
#define CCW_MAXB 4
#define CCW_MAX_C 160       // channels per branch half (Lite-HRNet: 20 / 40 / 80 / 160)
#define CCW_MAX_CT 320      // lhn_ccw_gate_fwd: concatenated channels
#define CCW_MAX_MID 40      // ... and hidden neurons; SpatialWeighting's J = C_b / 4 has the same bound
#define CCW_GATE_PX 4       // pooled pixels per workgroup of the gate kernel (they share every weight load)
#define CCW_DW_R 2          // pixels per pixel lane of a depthwise tile: tile = (256 / (C_b / 4)) * CCW_DW_R pixels of one sample
#define CCW_SH_R 8          // ... of a shuffle chunk (every workgroup repeats the fold and the MLP, so chunks are longer)

__device__ __forceinline__ float ccw_relu_sigmoid(float v) { return 1.f / (1.f + expf(-fmaxf(v, 0.f))); }
static inline int ccw_dw_tile_px(int C) { return (256 / (C >> 2)) * CCW_DW_R; }
static inline int ccw_dw_tiles(int H, int W, int C) { return (int)(((int64_t)H * W + ccw_dw_tile_px(C) - 1) / ccw_dw_tile_px(C)); }

struct CcwPool {
  lhn_view x[CCW_MAXB];
  int blk0[CCW_MAXB + 1];   // first workgroup of branch b
  int S[CCW_MAXB];          // lanes that share one output (a power of two <= 16): the window's pixels are dealt over them
  int coff[CCW_MAXB];       // first pooled channel of branch b
  int B, hm, wm, Ct;
  float* pooled;
};
// thread = (output (n, ph, pw, c4), sub) with sub fastest: S consecutive lanes of one wave add the window's pixels sub, sub + S, ..
// in turn and meet by xor-shuffles (a + b == b + a: every lane of the group ends with the same bits)
__global__ void __launch_bounds__(256) k_ccw_pool(CcwPool a) {
  int b = 0;
  while (b + 1 < a.B && (int)blockIdx.x >= a.blk0[b + 1]) ++b;
  const lhn_view& x = a.x[b];
  const int S = a.S[b], C4 = x.C >> 2, rh = x.H / a.hm, rw = x.W / a.wm, cnt = rh * rw;
  const int64_t r = (int64_t)(blockIdx.x - a.blk0[b]) * 256 + threadIdx.x;
  const int sub = (int)(r & (S - 1));
  const int64_t o = r / S, pix = o / C4;
  const int c4 = (int)(o - pix * C4);
  const bool live = pix < (int64_t)x.N * a.hm * a.wm;
  f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
  if (live) {
    const int n = (int)(pix / (a.hm * a.wm)), q = (int)(pix - (int64_t)n * a.hm * a.wm), ph = q / a.wm, pw = q - ph * a.wm;
    const int c = x.coff + 4 * c4;
    const Xf4 xf = lhn_load_xf(x, c);
    for (int k = sub; k < cnt; k += S) {
      const int i = k / rw, j = k - i * rw;
      acc += lhn_load_val(x, xf, ((int64_t)n * x.H + ph * rh + i) * x.W + pw * rw + j, n, c);
    }
  }
  for (int m = 1; m < S; m <<= 1) {
    acc.x += __shfl_xor(acc.x, m, 64); acc.y += __shfl_xor(acc.y, m, 64); acc.z += __shfl_xor(acc.z, m, 64); acc.w += __shfl_xor(acc.w, m, 64);
  }
  if (live && sub == 0) {
    const float d = (float)cnt;      // a division, not a reciprocal: constant maps pool to exactly their constant for any window
    *reinterpret_cast<f4*>(a.pooled + pix * a.Ct + a.coff[b] + 4 * c4) = (f4){acc.x / d, acc.y / d, acc.z / d, acc.w / d};
  }
}

// CrossResolutionWeighting's two 1x1 convolutions for CCW_GATE_PX pooled pixels per workgroup.  Hidden neuron j: one wave, lanes
// stride over the Ct inputs and meet in lhn_wave_sum; output channel c: one thread, the mid hidden values in order.
__global__ void __launch_bounds__(256) k_ccw_gate(const float* __restrict__ pooled, int64_t npix, int Ct, int mid, const float* __restrict__ w1,
                                                  const float* __restrict__ t1, int s1, const float* __restrict__ w2, const float* __restrict__ t2,
                                                  int s2, float* __restrict__ g) {
  __shared__ float sp[CCW_GATE_PX][CCW_MAX_CT], sh[CCW_GATE_PX][CCW_MAX_MID];
  const int64_t p0 = (int64_t)blockIdx.x * CCW_GATE_PX;
  const int np = (int)(npix - p0 < CCW_GATE_PX ? npix - p0 : CCW_GATE_PX), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < CCW_GATE_PX * Ct; i += 256) {
    const int q = i / Ct, c = i - q * Ct;
    sp[q][c] = q < np ? pooled[(p0 + q) * Ct + c] : 0.f;
  }
  __syncthreads();
  for (int j = wave; j < mid; j += 4) {
    float acc[CCW_GATE_PX];
#pragma unroll
    for (int q = 0; q < CCW_GATE_PX; ++q) acc[q] = 0.f;
    for (int c = lane; c < Ct; c += 64) {
      const float w = w1[j * Ct + c];
#pragma unroll
      for (int q = 0; q < CCW_GATE_PX; ++q) acc[q] += w * sp[q][c];
    }
#pragma unroll
    for (int q = 0; q < CCW_GATE_PX; ++q) acc[q] = lhn_wave_sum(acc[q]);
    if (lane == 0) {
      const float sc = t1[j], sf = t1[s1 + j], sl = t1[2 * s1 + j];
#pragma unroll
      for (int q = 0; q < CCW_GATE_PX; ++q) sh[q][j] = ccw_relu_sigmoid(lhn_lrelu(acc[q] * sc + sf, sl));
    }
  }
  __syncthreads();
  for (int c = tid; c < Ct; c += 256) {
    float acc[CCW_GATE_PX];
#pragma unroll
    for (int q = 0; q < CCW_GATE_PX; ++q) acc[q] = 0.f;
    for (int j = 0; j < mid; ++j) {
      const float w = w2[c * mid + j];
#pragma unroll
      for (int q = 0; q < CCW_GATE_PX; ++q) acc[q] += w * sh[q][j];
    }
    const float sc = t2[c], sf = t2[s2 + c], sl = t2[2 * s2 + c];
#pragma unroll
    for (int q = 0; q < CCW_GATE_PX; ++q)
      if (q < np) g[(p0 + q) * Ct + c] = ccw_relu_sigmoid(lhn_lrelu(acc[q] * sc + sf, sl));
  }
}

struct CcwDw {
  lhn_view x[CCW_MAXB], y[CCW_MAXB];
  const float* w[CCW_MAXB];
  int blk0[CCW_MAXB + 1];
  int T[CCW_MAXB];          // tiles per sample
  int goff[CCW_MAXB];       // first channel of branch b in g
  int64_t soff[CCW_MAXB];   // first float of branch b in scratch: [N][T][C_b]
  int B, hm, wm, Ct;
  const float* g;
  float* scratch;
};
// workgroup = (branch, sample, tile of (256 / C4) * CCW_DW_R pixels), thread = (c4, pixel lane) as in the elementwise kernels.  Gather
// form: nine taps of value(x2) * g per output (the maps are small and stay in cache); a tap outside the map contributes an exact zero
// (the PRODUCT is padded, so a table that shifts zero elsewhere does not show).
__global__ void __launch_bounds__(256) k_ccw_dw(CcwDw a) {
  __shared__ f4 red[256];
  int b = 0;
  while (b + 1 < a.B && (int)blockIdx.x >= a.blk0[b + 1]) ++b;
  const lhn_view &x = a.x[b], &y = a.y[b];
  const int T = a.T[b], r = blockIdx.x - a.blk0[b], n = r / T, tile = r - n * T;
  const int C4 = x.C >> 2, PL = 256 / C4, tid = threadIdx.x, c4 = tid % C4, pl = tid / C4;
  const int H = x.H, W = x.W, HW = H * W, rh = H / a.hm, rw = W / a.wm, TP = PL * CCW_DW_R;
  const int p0 = tile * TP, p1 = p0 + TP < HW ? p0 + TP : HW;
  const int cx = x.coff + 4 * c4, cy = y.coff + 4 * c4, cg = a.goff[b] + 4 * c4;
  f4 s = (f4){0.f, 0.f, 0.f, 0.f};
  if (pl < PL) {
    const Xf4 xf = lhn_load_xf(x, cx), yf = lhn_load_xf(y, cy);
    f4 wk[9];
    const float* wp = a.w[b] + (size_t)(4 * c4) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = (f4){wp[k], wp[9 + k], wp[18 + k], wp[27 + k]};
    for (int p = p0 + pl; p < p1; p += PL) {
      const int h = p / W, w = p - h * W;
      f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hh = h + kh - 1;
        if (hh < 0 || hh >= H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ww = w + kw - 1;
          if (ww < 0 || ww >= W) continue;
          const f4 gv = *reinterpret_cast<const f4*>(a.g + (((int64_t)n * a.hm + hh / rh) * a.wm + ww / rw) * a.Ct + cg);
          acc += wk[kh * 3 + kw] * (lhn_load_val(x, xf, ((int64_t)n * H + hh) * W + ww, n, cx) * gv);
        }
      }
      *reinterpret_cast<f4*>(y.data + ((int64_t)n * HW + p) * y.cstride + cy) = acc;
      s += lhn_apply_xf(acc, yf);
    }
  }
  red[tid] = s;
  __syncthreads();
  if (tid < C4) {
    f4 t = red[tid];
    for (int j = 1; j < PL; ++j) t += red[j * C4 + tid];
    *reinterpret_cast<f4*>(a.scratch + a.soff[b] + ((int64_t)n * T + tile) * x.C + 4 * tid) = t;
  }
}

struct CcwShuffle {
  lhn_view x1[CCW_MAXB], y[CCW_MAXB], out[CCW_MAXB];
  lhn_ccw_se se[CCW_MAXB];
  int blk0[CCW_MAXB + 1];
  int K[CCW_MAXB];          // pixel chunks per sample
  int T[CCW_MAXB];          // tiles per sample of the depthwise launch
  int64_t soff[CCW_MAXB];
  int B;
  const float* scratch;
};
// workgroup = (branch, sample, chunk of (256 / (C_b / 2)) * CCW_SH_R pixels).  Prologue: the sample's tile sums in tile order -> mean,
// then the SpatialWeighting MLP with the loops of k_se_fwd (k_att.hip, mode 1); body: k_shuffle2_fwd with the gate in LDS.
__global__ void __launch_bounds__(256) k_ccw_shuffle(CcwShuffle a) {
  __shared__ float sp[CCW_MAX_C], sh[CCW_MAX_MID], sg[CCW_MAX_C];
  int b = 0;
  while (b + 1 < a.B && (int)blockIdx.x >= a.blk0[b + 1]) ++b;
  const lhn_view &xa = a.x1[b], &xb = a.y[b], &dst = a.out[b];
  const lhn_ccw_se& se = a.se[b];
  const int K = a.K[b], T = a.T[b], r = blockIdx.x - a.blk0[b], n = r / K, chunk = r - n * K;
  const int C = xb.C, J = se.J, HW = dst.H * dst.W, tid = threadIdx.x;
  const float* part = a.scratch + a.soff[b] + (int64_t)n * T * C;
  for (int c = tid; c < C; c += 256) {
    float t = 0.f;
    for (int k = 0; k < T; ++k) t += part[(int64_t)k * C + c];
    sp[c] = t / (float)HW;
  }
  __syncthreads();
  for (int j = tid; j < J; j += 256) {
    float v = se.b1 ? se.b1[j] : 0.f;
    for (int c = 0; c < C; ++c) v += se.w1[j * C + c] * sp[c];
    sh[j] = 1.f / (1.f + expf(-fmaxf(v, 0.f)));
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float v = se.b2 ? se.b2[c] : 0.f;
    for (int j = 0; j < J; ++j) v += se.w2[c * J + j] * sh[j];
    sg[c] = 1.f / (1.f + expf(-fmaxf(v, 0.f)));
  }
  __syncthreads();
  const int C4 = dst.C >> 2, PL = 256 / C4, c4 = tid % C4, pl = tid / C4;
  if (pl >= PL) return;
  const int ca = xa.coff + 2 * c4, cb = xb.coff + 2 * c4;
  const Xf2 fa = load_xf2(xa, ca), fb = load_xf2(xb, cb);
  float ga[2] = {1.f, 1.f};
  if (xa.gate) { ga[0] = xa.gate[(size_t)n * xa.cstride + ca]; ga[1] = xa.gate[(size_t)n * xa.cstride + ca + 1]; }
  const float gb[2] = {sg[2 * c4], sg[2 * c4 + 1]};
  const int p0 = chunk * PL * CCW_SH_R, p1 = p0 + PL * CCW_SH_R < HW ? p0 + PL * CCW_SH_R : HW;
  for (int p = p0 + pl; p < p1; p += PL) {
    const size_t pix = (size_t)n * HW + p;
    const float2 ra = *reinterpret_cast<const float2*>(xa.data + pix * xa.cstride + ca);
    const float2 rb = *reinterpret_cast<const float2*>(xb.data + pix * xb.cstride + cb);
    f4 o;
    o.x = lhn_lrelu(ra.x * fa.sc[0] + fa.sh[0], fa.sl[0]) * ga[0];
    o.y = lhn_lrelu(rb.x * fb.sc[0] + fb.sh[0], fb.sl[0]) * gb[0];
    o.z = lhn_lrelu(ra.y * fa.sc[1] + fa.sh[1], fa.sl[1]) * ga[1];
    o.w = lhn_lrelu(rb.y * fb.sc[1] + fb.sh[1], fb.sl[1]) * gb[1];
    *reinterpret_cast<f4*>(dst.data + pix * dst.cstride + dst.coff + 4 * c4) = o;
  }
}

// What all four entry points ask of the branches' views v[0..B): 2..4 branches of one batch, ordered from the largest map to the
// smallest, every map an integer multiple of the last, at most CCW_MAX_C channels each (views hold multiples of 4, so C_b is even).
static bool ccw_branches_ok(const lhn_view* v, int B) {
  if (!v || B < 2 || B > CCW_MAXB) return false;
  for (int b = 0; b < B; ++b)      // (before any division by a map size)
    if (!lhn_view_ok(&v[b]) || !lhn_no_pend(&v[b]) || v[b].N != v[0].N || v[b].C > CCW_MAX_C) return false;
  const int hm = v[B - 1].H, wm = v[B - 1].W;
  for (int b = 0; b < B; ++b) {
    if (v[b].H % hm || v[b].W % wm) return false;
    if (b && (v[b].H > v[b - 1].H || v[b].W > v[b - 1].W)) return false;
  }
  return true;
}
static bool ccw_same_geometry(const lhn_view* u, const lhn_view* v, int B, int cmul) {
  for (int b = 0; b < B; ++b)
    if (!lhn_view_ok(&u[b]) || !lhn_no_pend(&u[b]) || u[b].N != v[b].N || u[b].H != v[b].H || u[b].W != v[b].W || u[b].C != cmul * v[b].C) return false;
  return true;
}
static bool ccw_overlap(const lhn_view& o, const lhn_view& i) { return o.data == i.data && o.coff < i.coff + i.C && i.coff < o.coff + o.C; }

extern "C" {

int64_t lhn_ccw_scratch_bytes(int N, int B, const int* H, const int* W, const int* C) {
  if (N < 1 || B < 2 || B > CCW_MAXB || !H || !W || !C) return 0;
  int64_t n = 0;
  for (int b = 0; b < B; ++b)
    if (H[b] < 1 || W[b] < 1 || C[b] < 4 || C[b] % 4 || C[b] > CCW_MAX_C) return 0;
  for (int b = 0; b < B; ++b) {
    if (H[b] % H[B - 1] || W[b] % W[B - 1] || (b && (H[b] > H[b - 1] || W[b] > W[b - 1]))) return 0;
    n += (int64_t)N * ccw_dw_tiles(H[b], W[b], C[b]) * C[b] * 4;
  }
  return n;
}

int lhn_ccw_pool_fwd(const lhn_view* x2, int B, float* pooled, void* stream) {
  LHN_CHECK_ARG(ccw_branches_ok(x2, B) && pooled, "lhn_ccw_pool_fwd: unsupported shape (2..4 branches, largest map first, integer ratios, C <= 160)");
  CcwPool a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.hm = x2[B - 1].H; a.wm = x2[B - 1].W; a.pooled = pooled;
  int64_t blk = 0;
  for (int b = 0; b < B; ++b) {
    LHN_CHECK_ARG(x2[b].data != pooled, "lhn_ccw_pool_fwd: unsupported shape (pooled overlaps an input)");
    a.x[b] = x2[b];
    a.coff[b] = a.Ct;
    a.Ct += x2[b].C;
    const int cnt = (x2[b].H / a.hm) * (x2[b].W / a.wm);
    int S = 1;
    while (S * 2 <= cnt && S < 16) S *= 2;
    a.S[b] = S;
    a.blk0[b] = (int)blk;
    blk += ((int64_t)x2[b].N * a.hm * a.wm * (x2[b].C >> 2) * S + 255) / 256;
    LHN_CHECK_ARG(blk < (1 << 30), "lhn_ccw_pool_fwd: unsupported shape (grid too large)");
  }
  for (int b = B; b <= CCW_MAXB; ++b) a.blk0[b] = (int)blk;
  hipLaunchKernelGGL(k_ccw_pool, dim3((unsigned)blk), dim3(256), 0, (hipStream_t)stream, a);
  LHN_CHECK_LAUNCH("lhn_ccw_pool_fwd");
  return 0;
}

int lhn_ccw_gate_fwd(const float* pooled, int64_t npix, int Ct, int mid, const float* w1, const float* t1, int t1_stride, const float* w2,
                     const float* t2, int t2_stride, float* g, void* stream) {
  LHN_CHECK_ARG(pooled && g && w1 && w2 && t1 && t2 && pooled != g, "lhn_ccw_gate_fwd: missing argument");
  LHN_CHECK_ARG(npix > 0 && npix < ((int64_t)1 << 31) && Ct > 0 && Ct <= CCW_MAX_CT && mid > 0 && mid <= CCW_MAX_MID && t1_stride >= mid && t2_stride >= Ct,
                "lhn_ccw_gate_fwd: unsupported shape (Ct = %d <= 320, mid = %d <= 40)", Ct, mid);
  hipLaunchKernelGGL(k_ccw_gate, dim3((unsigned)((npix + CCW_GATE_PX - 1) / CCW_GATE_PX)), dim3(256), 0, (hipStream_t)stream, pooled, npix, Ct,
                     mid, w1, t1, t1_stride, w2, t2, t2_stride, g);
  LHN_CHECK_LAUNCH("lhn_ccw_gate_fwd");
  return 0;
}

int lhn_ccw_dw_fwd(const lhn_view* x2, int B, const float* g, const float* const* w, const lhn_view* y, void* scratch, void* stream) {
  LHN_CHECK_ARG(ccw_branches_ok(x2, B) && y && ccw_same_geometry(y, x2, B, 1) && g && w,
                "lhn_ccw_dw_fwd: unsupported shape (2..4 branches, largest map first, integer ratios, C <= 160, y like x2)");
  LHN_CHECK_ARG(scratch, "lhn_ccw_dw_fwd: unsupported shape (no scratch: lhn_ccw_scratch_bytes)");
  CcwDw a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.hm = x2[B - 1].H; a.wm = x2[B - 1].W; a.g = g; a.scratch = static_cast<float*>(scratch);
  int64_t blk = 0, so = 0;
  for (int b = 0; b < B; ++b) {
    LHN_CHECK_ARG(w[b] && y[b].data != g, "lhn_ccw_dw_fwd: missing weights of branch %d", b);
    for (int k = 0; k < B; ++k) {
      LHN_CHECK_ARG(!ccw_overlap(y[b], x2[k]), "lhn_ccw_dw_fwd: unsupported shape (y[%d] overlaps x2[%d] in the same buffer)", b, k);
      LHN_CHECK_ARG(k == b || !ccw_overlap(y[b], y[k]), "lhn_ccw_dw_fwd: unsupported shape (y[%d] overlaps y[%d])", b, k);
    }
    a.x[b] = x2[b]; a.y[b] = y[b]; a.w[b] = w[b];
    a.goff[b] = a.Ct;
    a.Ct += x2[b].C;
    a.T[b] = ccw_dw_tiles(x2[b].H, x2[b].W, x2[b].C);
    a.soff[b] = so;
    so += (int64_t)x2[b].N * a.T[b] * x2[b].C;
    a.blk0[b] = (int)blk;
    blk += (int64_t)x2[b].N * a.T[b];
    LHN_CHECK_ARG(blk < (1 << 30) && (int64_t)x2[b].H * x2[b].W < (1 << 30), "lhn_ccw_dw_fwd: unsupported shape (grid too large)");
  }
  for (int b = B; b <= CCW_MAXB; ++b) a.blk0[b] = (int)blk;
  hipLaunchKernelGGL(k_ccw_dw, dim3((unsigned)blk), dim3(256), 0, (hipStream_t)stream, a);
  LHN_CHECK_LAUNCH("lhn_ccw_dw_fwd");
  return 0;
}

int lhn_ccw_shuffle_fwd(const lhn_view* x1, const lhn_view* y, int B, const lhn_ccw_se* se, const void* scratch, const lhn_view* out,
                        void* stream) {
  LHN_CHECK_ARG(ccw_branches_ok(y, B) && x1 && out && se && ccw_same_geometry(x1, y, B, 1) && ccw_same_geometry(out, y, B, 2),
                "lhn_ccw_shuffle_fwd: unsupported shape (2..4 branches, largest map first, integer ratios, C <= 160, x1 like y, out twice as wide)");
  LHN_CHECK_ARG(scratch, "lhn_ccw_shuffle_fwd: unsupported shape (no scratch: lhn_ccw_scratch_bytes)");
  CcwShuffle a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.scratch = static_cast<const float*>(scratch);
  int64_t blk = 0, so = 0;
  for (int b = 0; b < B; ++b) {
    LHN_CHECK_ARG(se[b].w1 && se[b].w2 && se[b].J >= 1 && se[b].J <= CCW_MAX_MID, "lhn_ccw_shuffle_fwd: unsupported shape (branch %d: J = %d, 1..40)", b, se[b].J);
    for (int k = 0; k < B; ++k)
      LHN_CHECK_ARG(!ccw_overlap(out[b], x1[k]) && !ccw_overlap(out[b], y[k]) && (k == b || !ccw_overlap(out[b], out[k])),
                    "lhn_ccw_shuffle_fwd: unsupported shape (out[%d] overlaps a view of branch %d in the same buffer)", b, k);
    a.x1[b] = x1[b]; a.y[b] = y[b]; a.out[b] = out[b]; a.se[b] = se[b];
    a.T[b] = ccw_dw_tiles(y[b].H, y[b].W, y[b].C);
    a.soff[b] = so;
    so += (int64_t)y[b].N * a.T[b] * y[b].C;
    const int64_t chunk = (256 / (out[b].C >> 2)) * CCW_SH_R, HW = (int64_t)y[b].H * y[b].W;
    LHN_CHECK_ARG(HW < (1 << 30), "lhn_ccw_shuffle_fwd: unsupported shape (map too large)");
    a.K[b] = (int)((HW + chunk - 1) / chunk);
    a.blk0[b] = (int)blk;
    blk += (int64_t)y[b].N * a.K[b];
    LHN_CHECK_ARG(blk < (1 << 30), "lhn_ccw_shuffle_fwd: unsupported shape (grid too large)");
  }
  for (int b = B; b <= CCW_MAXB; ++b) a.blk0[b] = (int)blk;
  hipLaunchKernelGGL(k_ccw_shuffle, dim3((unsigned)blk), dim3(256), 0, (hipStream_t)stream, a);
  LHN_CHECK_LAUNCH("lhn_ccw_shuffle_fwd");
  return 0;
}

int lhn_shuffle2_fwd(const lhn_view* a, const lhn_view* b, const lhn_view* dst, void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(a) && lhn_view_ok(b) && lhn_view_ok(dst) && lhn_no_pend(a) && lhn_no_pend(b), "lhn_shuffle2_fwd: bad views");
  LHN_CHECK_ARG(a->C == b->C && dst->C == 2 * a->C && a->C % 2 == 0 && a->coff % 2 == 0 && b->coff % 2 == 0 && a->cstride % 2 == 0 &&
                    b->cstride % 2 == 0 && dst->C <= 1024,
                "lhn_shuffle2_fwd: channels %d + %d -> %d", a->C, b->C, dst->C);
  LHN_CHECK_ARG(a->N == dst->N && a->H == dst->H && a->W == dst->W && b->N == dst->N && b->H == dst->H && b->W == dst->W,
                "lhn_shuffle2_fwd: geometry");
  hipLaunchKernelGGL(k_shuffle2_fwd, dim3(grid_cap((int64_t)dst->N * dst->H, 8)), dim3(256), 0, (hipStream_t)stream, *a, *b, *dst);
  LHN_CHECK_LAUNCH("lhn_shuffle2_fwd");
  return 0;
}
int lhn_shuffle2_bwd(const lhn_view* a, const lhn_view* b, const lhn_view* dst, const float* ddst, float* da, int acc_a, float* db,
                     int acc_b, void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(a) && lhn_view_ok(b) && lhn_view_ok(dst) && ddst && (da || db), "lhn_shuffle2_bwd: bad args");
  LHN_CHECK_ARG(a->C == b->C && dst->C == 2 * a->C && a->C % 2 == 0 && dst->C <= 1024, "lhn_shuffle2_bwd: channels");
  hipLaunchKernelGGL(k_shuffle2_bwd, dim3(grid_cap((int64_t)dst->N * dst->H, 8)), dim3(256), 0, (hipStream_t)stream, *a, *b, *dst, ddst,
                     da, acc_a, db, acc_b);
  LHN_CHECK_LAUNCH("lhn_shuffle2_bwd");
  return 0;
}
int lhn_ew_mul_bwd(const lhn_view* src, const lhn_view* other, const lhn_view* dst, const float* ddst, float* dsrc, int accumulate,
                   void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(src) && lhn_view_ok(other) && lhn_view_ok(dst) && ddst && dsrc && src->C == dst->C && other->C == dst->C &&
                    src->C <= 1024 && lhn_no_pend(src) && lhn_no_pend(other),
                "lhn_ew_mul_bwd: bad args");
  LHN_CHECK_ARG(dst->H % src->H == 0 && dst->W % src->W == 0, "lhn_ew_mul_bwd: non-integer upsample");
  hipLaunchKernelGGL(k_ew_mul_bwd, dim3(grid_cap((int64_t)src->N * src->H, 8)), dim3(256), 0, (hipStream_t)stream, *src, *other, *dst,
                     ddst, dsrc, accumulate);
  LHN_CHECK_LAUNCH("lhn_ew_mul_bwd");
  return 0;
}
int lhn_bilinear_bwd(const lhn_view* src, const lhn_view* dst, const float* ddst, float* dsrc, int accumulate, float out_slope,
                     void* stream) {
  LHN_CHECK_ARG(lhn_view_ok(src) && lhn_view_ok(dst) && ddst && dsrc && src->C == dst->C && src->C <= 1024 && lhn_no_pend(src),
                "lhn_bilinear_bwd: bad args");
  LHN_CHECK_ARG(src->H <= dst->H && src->W <= dst->W, "lhn_bilinear_bwd: the source must not be larger than the destination");
  LHN_CHECK_ARG(out_slope != LHN_SLOPE_SILU && out_slope != LHN_SLOPE_RELU_SIGMOID,
                "lhn_bilinear_bwd: SiLU / ReLU-sigmoid need a single same-size source (lhn_ew_bwd3)");
  hipLaunchKernelGGL(k_bilinear_bwd, dim3(grid_cap((int64_t)src->N * src->H, 8)), dim3(256), 0, (hipStream_t)stream, *src, *dst, ddst,
                     dsrc, accumulate, out_slope);
  LHN_CHECK_LAUNCH("lhn_bilinear_bwd");
  return 0;
}
}  // extern "C"
