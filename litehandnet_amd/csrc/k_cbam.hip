// CBAM (reference attention.py:234-294) between its `pre` convolutions and its final ReLU -- the one attention of this library
// whose gate is per PIXEL as well as per (sample, channel).  With p = the value of pre's output (lazy: raw + table), r = the value
// of residual_conv(x), J = C / 16:
//   avg, mx = mean / max over the map of p (first arg-max pixel kept)          k_cbam_pool (+ the fold in k_cbam_mlp_fwd)
//   g = sigmoid(W2 relu(W1 avg) + W2 relu(W1 mx))                              k_cbam_mlp_fwd, one workgroup per sample
//   u = g p;  s0 = mean_c u, s1 = max_c u (first arg-max channel kept)         k_cbam_spatial
//   a = sigmoid(conv7x7(s));  out = relu(a u + r)                              k_cbam_apply (s tile + 3-pixel halo in LDS)
// backward, dz = dout [out > 0]:
//   dr = dz;  dq = a (1 - a) sum_c dz u                                        k_cbam_dq
//   ds = W7 mirrored over dq;  du = a dz + ds0 / C + [c == argmax] ds1;        k_cbam_du (dq and s halos in LDS; per-workgroup
//   dW7 = sum dq (x) s;  dg = sum_px du p                                        partials of dW7 and dg)
//   dg -> sigmoid -> both MLP paths -> dW1, dW2 (per sample), davg, dmx        k_cbam_mlp_bwd
//   dp = g du + davg / HW + [px == argmax] dmx   (in place over du)            k_cbam_dp
// du is written into the gradient buffer of p and rewritten in place as dp, the gradient with respect to p's VALUE: the ordinary
// convolution + BatchNorm backward of `pre` takes it from there (one extra read-modify-write pass over that buffer).
// No float atomics: every sum across workgroups is a store into the workgroup's own slot of caller-owned memory and a fold in
// fixed order (k_cbam_fold, or the head of the kernel that consumes it), so results repeat bit for bit in every mode.
#include "lhn_common.h"

#define CB_TH 8
#define CB_TW 32
#define CB_HH (CB_TH + 6)
#define CB_HW (CB_TW + 6)
#define CB_MAXSPLIT 16
#define CB_NOIDX 0x7fffffff

struct CbamLayout {
  // save (written by the forward, read by the backward), in floats
  int64_t avg, mx, amax, hid, g, s, cidx, a, ppart, save_total;
  // backward scratch, in floats
  int64_t dq, w7part, dgpart, davg, dmx, w1part, w2part, scratch_total;
  int S, ntx, nty;
};
static inline int64_t cb_al(int64_t n) { return (n + 3) / 4 * 4; }
static CbamLayout cbam_layout(int N, int H, int W, int C) {
  CbamLayout L;
  const int64_t HW = (int64_t)H * W, J = C / 16, NC = (int64_t)N * C;
  int64_t S = (HW + 1023) / 1024;
  L.S = (int)(S < 1 ? 1 : (S > CB_MAXSPLIT ? CB_MAXSPLIT : S));
  L.ntx = (W + CB_TW - 1) / CB_TW;
  L.nty = (H + CB_TH - 1) / CB_TH;
  const int64_t NT = (int64_t)N * L.ntx * L.nty;
  int64_t o = 0;
  L.avg = o; o += cb_al(NC);
  L.mx = o; o += cb_al(NC);
  L.amax = o; o += cb_al(NC);
  L.hid = o; o += cb_al(N * 2 * J);
  L.g = o; o += cb_al(NC);
  L.s = o; o += cb_al(N * HW * 2);
  L.cidx = o; o += cb_al(N * HW);
  L.a = o; o += cb_al(N * HW);
  L.ppart = o; o += cb_al(NC * L.S * 3);
  L.save_total = o;
  o = 0;
  L.dq = o; o += cb_al(N * HW);
  L.w7part = o; o += cb_al(NT * 98);
  L.dgpart = o; o += cb_al(NT * C);
  L.davg = o; o += cb_al(NC);
  L.dmx = o; o += cb_al(NC);
  L.w1part = o; o += cb_al(NC * J);
  L.w2part = o; o += cb_al(NC * J);
  L.scratch_total = o;
  return L;
}

__device__ __forceinline__ float cb_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
// (value, index) pairs: the larger value wins, equal values keep the smaller index
__device__ __forceinline__ void cb_max_merge(float& m, int& mi, float v, int vi) {
  if (v > m || (v == m && vi < mi)) {
    m = v;
    mi = vi;
  }
}

// ---------------------------------------------------------------- forward
// grid N * S workgroups: split sp of sample n reduces its pixels [lo, hi) for all channels.  Thread = (float4 channel group
// c4 = tid % C4, pixel lane pl = tid / C4), the lanes meet in LDS in lane order.  ppart[(n * S + sp) * 3 + {sum, max, index}][C]
__global__ void __launch_bounds__(256) k_cbam_pool(lhn_view p, float* __restrict__ ppart, int S) {
  __shared__ f4 ssum[256], smax[256];
  __shared__ int sidx[256 * 4];
  const int C = p.C, C4 = C / 4, PL = 256 / C4, tid = threadIdx.x, c4 = tid % C4, pl = tid / C4;
  const int n = blockIdx.x / S, sp = blockIdx.x % S, HW = p.H * p.W;
  const int chunk = (HW + S - 1) / S, lo = sp * chunk, hi = min(HW, lo + chunk);
  f4 sum = (f4){0.f, 0.f, 0.f, 0.f};
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int mi[4] = {CB_NOIDX, CB_NOIDX, CB_NOIDX, CB_NOIDX};
  if (pl < PL) {
    const int ca = p.coff + 4 * c4;
    const Xf4 t = lhn_load_xf(p, ca);
    for (int px = lo + pl; px < hi; px += PL) {
      const f4 v = lhn_load_val(p, t, (int64_t)n * HW + px, n, ca);
      sum += v;
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (vv[j] > m[j]) {      // pixels ascend within a lane: strict > keeps the first
          m[j] = vv[j];
          mi[j] = px;
        }
    }
  }
  ssum[tid] = sum;
  smax[tid] = (f4){m[0], m[1], m[2], m[3]};
#pragma unroll
  for (int j = 0; j < 4; ++j) sidx[tid * 4 + j] = mi[j];
  __syncthreads();
  if (tid < C4) {
    for (int l = 1; l < PL; ++l) {
      const int o = l * C4 + tid;
      sum += ssum[o];
      const f4 v = smax[o];
      cb_max_merge(m[0], mi[0], v.x, sidx[o * 4]);
      cb_max_merge(m[1], mi[1], v.y, sidx[o * 4 + 1]);
      cb_max_merge(m[2], mi[2], v.z, sidx[o * 4 + 2]);
      cb_max_merge(m[3], mi[3], v.w, sidx[o * 4 + 3]);
    }
    float* dst = ppart + ((int64_t)n * S + sp) * 3 * C + 4 * tid;
    *reinterpret_cast<f4*>(dst) = sum;
    *reinterpret_cast<f4*>(dst + C) = (f4){m[0], m[1], m[2], m[3]};
    *reinterpret_cast<int4*>(dst + 2 * C) = make_int4(mi[0], mi[1], mi[2], mi[3]);
  }
}

// one workgroup per sample: fold the splits in order, both paths of the shared MLP, the gate.  hid[n][2][J] = the hidden rows after
// their ReLU (mean path, max path)
__global__ void __launch_bounds__(256) k_cbam_mlp_fwd(const float* __restrict__ ppart, int S, const float* __restrict__ w1,
                                                      const float* __restrict__ w2, float* __restrict__ avg, float* __restrict__ mx,
                                                      int* __restrict__ amax, float* __restrict__ hid, float* __restrict__ g, int C,
                                                      int HW) {
  __shared__ float sa[256], sm[256], sh[32];
  const int n = blockIdx.x, J = C / 16, tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) {
    float sum = 0.f, m = -INFINITY;
    int mi = CB_NOIDX;
    for (int sp = 0; sp < S; ++sp) {
      const float* src = ppart + ((int64_t)n * S + sp) * 3 * C + c;
      sum += src[0];
      cb_max_merge(m, mi, src[C], reinterpret_cast<const int*>(src)[2 * C]);
    }
    const float a = sum / (float)HW;
    sa[c] = a;
    sm[c] = m;
    avg[(int64_t)n * C + c] = a;
    mx[(int64_t)n * C + c] = m;
    amax[(int64_t)n * C + c] = mi;
  }
  __syncthreads();
  if (tid < 2 * J) {
    const int path = tid / J, j = tid - path * J;
    const float* src = path ? sm : sa;
    float v = 0.f;
    for (int c = 0; c < C; ++c) v += w1[j * C + c] * src[c];
    v = fmaxf(v, 0.f);
    sh[tid] = v;
    hid[(int64_t)n * 2 * J + tid] = v;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float va = 0.f, vm = 0.f;
    for (int j = 0; j < J; ++j) {
      va += w2[c * J + j] * sh[j];
      vm += w2[c * J + j] * sh[J + j];
    }
    g[(int64_t)n * C + c] = cb_sigmoid(va + vm);
  }
}

// LP lanes (a power of two >= C / 4) share one pixel, 256 / LP pixels per workgroup and round; the channel reduction is a shuffle
// butterfly inside the wave.  s[n][px][{mean, max}], cidx[n][px] = first channel of the maximum
template <int LP>
__global__ void __launch_bounds__(256) k_cbam_spatial(lhn_view p, const float* __restrict__ g, float* __restrict__ s,
                                                      int* __restrict__ cidx, int64_t total) {
  constexpr int PPB = 256 / LP;
  const int C = p.C, C4 = C / 4, HW = p.H * p.W, lc = threadIdx.x % LP, slot = threadIdx.x / LP;
  const bool live = lc < C4;
  const int ca = p.coff + 4 * (live ? lc : 0);
  const Xf4 t = lhn_load_xf(p, ca);
  const float inv_c = 1.f / (float)C;
  for (int64_t base = (int64_t)blockIdx.x * PPB; base < total; base += (int64_t)gridDim.x * PPB) {
    const int64_t gp = base + slot;
    const bool on = live && gp < total;
    float sum = 0.f, m = -INFINITY;
    int mi = CB_NOIDX;
    if (on) {
      const int n = (int)(gp / HW);
      const f4 u = lhn_load_val(p, t, gp, n, ca) * *reinterpret_cast<const f4*>(g + (int64_t)n * C + 4 * lc);
      sum = (u.x + u.y) + (u.z + u.w);
      cb_max_merge(m, mi, u.x, 4 * lc);
      cb_max_merge(m, mi, u.y, 4 * lc + 1);
      cb_max_merge(m, mi, u.z, 4 * lc + 2);
      cb_max_merge(m, mi, u.w, 4 * lc + 3);
    }
#pragma unroll
    for (int o = 1; o < LP; o <<= 1) {
      sum += __shfl_xor(sum, o, 64);
      const float om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      cb_max_merge(m, mi, om, oi);
    }
    if (lc == 0 && gp < total) {
      *reinterpret_cast<float2*>(s + gp * 2) = make_float2(sum * inv_c, m);
      cidx[gp] = mi;
    }
  }
}

// one workgroup per 8 x 32 tile of one sample (grid: tiles, N)
__global__ void __launch_bounds__(256) k_cbam_apply(lhn_view p, lhn_view r, lhn_view out, const float* __restrict__ g,
                                                    const float* __restrict__ s, const float* __restrict__ w7, float* __restrict__ a,
                                                    int ntx) {
  __shared__ float sw[98], ss[2][CB_HH][CB_HW], sa[256];
  const int tid = threadIdx.x, n = blockIdx.y, H = p.H, W = p.W, HW = H * W;
  const int h0 = (blockIdx.x / ntx) * CB_TH, w0 = (blockIdx.x % ntx) * CB_TW;
  if (tid < 98) sw[tid] = w7[tid];
  for (int i = tid; i < CB_HH * CB_HW; i += 256) {
    const int lh = i / CB_HW, lw = i - lh * CB_HW, hh = h0 + lh - 3, ww = w0 + lw - 3;
    float2 v = make_float2(0.f, 0.f);
    if (hh >= 0 && hh < H && ww >= 0 && ww < W) v = *reinterpret_cast<const float2*>(s + ((int64_t)n * HW + hh * W + ww) * 2);
    ss[0][lh][lw] = v.x;
    ss[1][lh][lw] = v.y;
  }
  __syncthreads();
  {
    const int th = tid / CB_TW, tw = tid % CB_TW;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kh = 0; kh < 7; ++kh)
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) acc += sw[j * 49 + kh * 7 + kw] * ss[j][th + kh][tw + kw];
    const float av = cb_sigmoid(acc);
    sa[tid] = av;
    if (h0 + th < H && w0 + tw < W) a[(int64_t)n * HW + (h0 + th) * W + w0 + tw] = av;
  }
  __syncthreads();
  const int C = p.C, C4 = C / 4, PL = 256 / C4, c4 = tid % C4, pl = tid / C4;
  if (pl >= PL) return;
  const int cp = p.coff + 4 * c4, cr = r.coff + 4 * c4;
  const Xf4 tp = lhn_load_xf(p, cp), tr = lhn_load_xf(r, cr);
  const f4 g4 = *reinterpret_cast<const f4*>(g + (int64_t)n * C + 4 * c4);
  for (int q = pl; q < CB_TH * CB_TW; q += PL) {
    const int h = h0 + q / CB_TW, w = w0 + q % CB_TW;
    if (h >= H || w >= W) continue;
    const int64_t px = (int64_t)n * HW + h * W + w;
    const f4 u = lhn_load_val(p, tp, px, n, cp) * g4;
    const f4 z = sa[q] * u + lhn_load_val(r, tr, px, n, cr);
    *reinterpret_cast<f4*>(out.data + px * out.cstride + out.coff + 4 * c4) =
        (f4){fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
  }
}

// ---------------------------------------------------------------- backward
// dz = dout [out > 0] -> dr (stored with r's geometry); dq = a (1 - a) sum_c dz u.  Lane layout of k_cbam_spatial.
template <int LP>
__global__ void __launch_bounds__(256) k_cbam_dq(lhn_view p, lhn_view out, const float* __restrict__ dout, const float* __restrict__ g,
                                                 const float* __restrict__ a, float* __restrict__ dq, float* __restrict__ dr, int rcs,
                                                 int rcoff, int64_t total) {
  constexpr int PPB = 256 / LP;
  const int C = p.C, C4 = C / 4, HW = p.H * p.W, lc = threadIdx.x % LP, slot = threadIdx.x / LP;
  const bool live = lc < C4;
  const int ca = p.coff + 4 * (live ? lc : 0);
  const Xf4 t = lhn_load_xf(p, ca);
  for (int64_t base = (int64_t)blockIdx.x * PPB; base < total; base += (int64_t)gridDim.x * PPB) {
    const int64_t gp = base + slot;
    float sum = 0.f;
    if (live && gp < total) {
      const int n = (int)(gp / HW);
      const int64_t oo = gp * out.cstride + out.coff + 4 * lc;
      const f4 ov = *reinterpret_cast<const f4*>(out.data + oo);
      f4 dz = *reinterpret_cast<const f4*>(dout + oo);
      dz = (f4){ov.x > 0.f ? dz.x : 0.f, ov.y > 0.f ? dz.y : 0.f, ov.z > 0.f ? dz.z : 0.f, ov.w > 0.f ? dz.w : 0.f};
      *reinterpret_cast<f4*>(dr + gp * rcs + rcoff + 4 * lc) = dz;
      const f4 u = lhn_load_val(p, t, gp, n, ca) * *reinterpret_cast<const f4*>(g + (int64_t)n * C + 4 * lc);
      sum = (dz.x * u.x + dz.y * u.y) + (dz.z * u.z + dz.w * u.w);
    }
#pragma unroll
    for (int o = 1; o < LP; o <<= 1) sum += __shfl_xor(sum, o, 64);
    if (lc == 0 && gp < total) {
      const float av = a[gp];
      dq[gp] = av * (1.f - av) * sum;
    }
  }
}

// one workgroup per 8 x 32 tile of one sample (grid: tiles, N): ds from the dq halo, this tile's part of dW7 and of dg into the
// workgroup's own slots, du into the gradient buffer of p
__global__ void __launch_bounds__(256) k_cbam_du(lhn_view p, lhn_view out, const float* __restrict__ dout, const float* __restrict__ g,
                                                 const float* __restrict__ s, const float* __restrict__ a, const int* __restrict__ cidx,
                                                 const float* __restrict__ dq, const float* __restrict__ w7, float* __restrict__ dp,
                                                 float* __restrict__ w7part, float* __restrict__ dgpart, int ntx) {
  __shared__ float sw[98], ss[2][CB_HH][CB_HW], sdq[CB_HH][CB_HW], sd0[256], sd1[256], sa[256];
  __shared__ int sci[256];
  __shared__ f4 red[256];
  const int tid = threadIdx.x, n = blockIdx.y, H = p.H, W = p.W, HW = H * W;
  const int h0 = (blockIdx.x / ntx) * CB_TH, w0 = (blockIdx.x % ntx) * CB_TW;
  const int64_t tile = (int64_t)n * gridDim.x + blockIdx.x;
  if (tid < 98) sw[tid] = w7[tid];
  for (int i = tid; i < CB_HH * CB_HW; i += 256) {
    const int lh = i / CB_HW, lw = i - lh * CB_HW, hh = h0 + lh - 3, ww = w0 + lw - 3;
    float2 v = make_float2(0.f, 0.f);
    float d = 0.f;
    if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
      const int64_t px = (int64_t)n * HW + hh * W + ww;
      v = *reinterpret_cast<const float2*>(s + px * 2);
      d = dq[px];
    }
    ss[0][lh][lw] = v.x;
    ss[1][lh][lw] = v.y;
    sdq[lh][lw] = d;
  }
  __syncthreads();
  {
    const int th = tid / CB_TW, tw = tid % CB_TW;
    float d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int kh = 0; kh < 7; ++kh)
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) {
        const float d = sdq[th + 6 - kh][tw + 6 - kw];      // dq[h - kh + 3][w - kw + 3]: the taps mirrored
        d0 += sw[kh * 7 + kw] * d;
        d1 += sw[49 + kh * 7 + kw] * d;
      }
    const bool in = h0 + th < H && w0 + tw < W;
    const int64_t px = (int64_t)n * HW + (h0 + th) * W + w0 + tw;
    sd0[tid] = d0 / (float)p.C;
    sd1[tid] = d1;
    sa[tid] = in ? a[px] : 0.f;
    sci[tid] = in ? cidx[px] : -1;
  }
  if (tid < 98) {      // dW7[j][kh][kw] over this tile: dq is zero outside the map, s too
    const int j = tid / 49, kh = (tid % 49) / 7, kw = tid % 7;
    float acc = 0.f;
    for (int q = 0; q < CB_TH * CB_TW; ++q) {
      const int th = q / CB_TW, tw = q % CB_TW;
      acc += sdq[th + 3][tw + 3] * ss[j][th + kh][tw + kw];
    }
    w7part[tile * 98 + tid] = acc;
  }
  __syncthreads();
  const int C = p.C, C4 = C / 4, PL = 256 / C4, c4 = tid % C4, pl = tid / C4;
  f4 dg = (f4){0.f, 0.f, 0.f, 0.f};
  if (pl < PL) {
    const int cp = p.coff + 4 * c4;
    const Xf4 tp = lhn_load_xf(p, cp);
    for (int q = pl; q < CB_TH * CB_TW; q += PL) {
      const int h = h0 + q / CB_TW, w = w0 + q % CB_TW;
      if (h >= H || w >= W) continue;
      const int64_t px = (int64_t)n * HW + h * W + w, oo = px * out.cstride + out.coff + 4 * c4;
      const f4 ov = *reinterpret_cast<const f4*>(out.data + oo);
      f4 dz = *reinterpret_cast<const f4*>(dout + oo);
      dz = (f4){ov.x > 0.f ? dz.x : 0.f, ov.y > 0.f ? dz.y : 0.f, ov.z > 0.f ? dz.z : 0.f, ov.w > 0.f ? dz.w : 0.f};
      const int k = sci[q] - 4 * c4;
      const float d1 = sd1[q];
      f4 du = sa[q] * dz + sd0[q];
      du += (f4){k == 0 ? d1 : 0.f, k == 1 ? d1 : 0.f, k == 2 ? d1 : 0.f, k == 3 ? d1 : 0.f};
      *reinterpret_cast<f4*>(dp + px * p.cstride + cp) = du;
      dg += du * lhn_load_val(p, tp, px, n, cp);
    }
  }
  red[tid] = dg;
  __syncthreads();
  if (tid < C4) {
    for (int l = 1; l < PL; ++l) dg += red[l * C4 + tid];
    *reinterpret_cast<f4*>(dgpart + tile * C + 4 * tid) = dg;
  }
}

// one workgroup per sample: fold dg over the sample's tiles in order, back through the sigmoid and both MLP paths.  The weight
// gradients of this sample go to w1part[n][J][C] / w2part[n][C][J]
__global__ void __launch_bounds__(256) k_cbam_mlp_bwd(const float* __restrict__ dgpart, int ntiles, const float* __restrict__ w1,
                                                      const float* __restrict__ w2, const float* __restrict__ avg,
                                                      const float* __restrict__ mx, const float* __restrict__ hid,
                                                      const float* __restrict__ g, float* __restrict__ davg, float* __restrict__ dmx,
                                                      float* __restrict__ w1part, float* __restrict__ w2part, int C) {
  __shared__ float spre[256], sa[256], sm[256], sh[32], sdh[32];
  const int n = blockIdx.x, J = C / 16, tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) {
    float d = 0.f;
    for (int t = 0; t < ntiles; ++t) d += dgpart[((int64_t)n * ntiles + t) * C + c];
    const float gv = g[(int64_t)n * C + c];
    spre[c] = d * gv * (1.f - gv);
    sa[c] = avg[(int64_t)n * C + c];
    sm[c] = mx[(int64_t)n * C + c];
  }
  if (tid < 2 * J) sh[tid] = hid[(int64_t)n * 2 * J + tid];
  __syncthreads();
  if (tid < 2 * J) {
    const int j = tid % J;
    float d = 0.f;
    for (int c = 0; c < C; ++c) d += w2[c * J + j] * spre[c];
    sdh[tid] = sh[tid] > 0.f ? d : 0.f;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float da = 0.f, dm = 0.f;
    for (int j = 0; j < J; ++j) {
      da += w1[j * C + c] * sdh[j];
      dm += w1[j * C + c] * sdh[J + j];
    }
    davg[(int64_t)n * C + c] = da;
    dmx[(int64_t)n * C + c] = dm;
  }
  for (int i = tid; i < C * J; i += 256) {
    const int c = i / J, j = i - c * J;
    w2part[(int64_t)n * C * J + i] = spre[c] * (sh[j] + sh[J + j]);
    const int jj = i / C, cc = i - jj * C;
    w1part[(int64_t)n * C * J + i] = sdh[jj] * sa[cc] + sdh[J + jj] * sm[cc];
  }
}

// dst[i] += part[0][i] + part[1][i] + ... in that order (dst: the parameter's slice of the flat gradient buffer)
__global__ void __launch_bounds__(256) k_cbam_fold(const float* __restrict__ part, int K, int count, float* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc += part[(int64_t)k * count + i];
  dst[i] += acc;
}

// dp = g du + davg / HW + [px == argmax] dmx, in place over du
__global__ void __launch_bounds__(256) k_cbam_dp(float* __restrict__ dp, int cs, int coff, const float* __restrict__ g,
                                                 const float* __restrict__ davg, const float* __restrict__ dmx,
                                                 const int* __restrict__ amax, int C, int HW, int64_t total4) {
  const int C4 = C / 4;
  const float inv = 1.f / (float)HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int64_t gp = i / C4;
    const int c4 = (int)(i - gp * C4), n = (int)(gp / HW), px = (int)(gp - (int64_t)n * HW);
    const int64_t nc = (int64_t)n * C + 4 * c4;
    f4* d = reinterpret_cast<f4*>(dp + gp * cs + coff + 4 * c4);
    const f4 g4 = *reinterpret_cast<const f4*>(g + nc), da = *reinterpret_cast<const f4*>(davg + nc);
    const f4 dm = *reinterpret_cast<const f4*>(dmx + nc);
    const int4 am = *reinterpret_cast<const int4*>(amax + nc);
    f4 v = g4 * *d + da * inv;
    v += (f4){am.x == px ? dm.x : 0.f, am.y == px ? dm.y : 0.f, am.z == px ? dm.z : 0.f, am.w == px ? dm.w : 0.f};
    *d = v;
  }
}

// ---------------------------------------------------------------- entry points
static int cbam_args_ok(const char* who, const lhn_view* p, const lhn_view* r, const lhn_view* out) {
  LHN_CHECK_ARG(lhn_view_ok(p) && lhn_view_ok(r) && lhn_view_ok(out) && lhn_no_pend(p) && lhn_no_pend(r) && lhn_no_pend(out),
                "%s: bad view", who);
  LHN_CHECK_ARG(p->C % 16 == 0 && p->C <= 256, "%s: C=%d (a multiple of 16 -- the MLP has C / 16 hidden neurons -- and <= 256)", who,
                p->C);
  LHN_CHECK_ARG(r->C == p->C && out->C == p->C && r->N == p->N && out->N == p->N && r->H == p->H && out->H == p->H && r->W == p->W &&
                    out->W == p->W, "%s: p, r and out differ in shape", who);
  LHN_CHECK_ARG((int64_t)p->H * p->W < (1 << 30), "%s: map of %d x %d pixels", who, p->H, p->W);
  return 0;
}

extern "C" int lhn_cbam_layout(int N, int H, int W, int C, int64_t* save_off, int64_t* scratch_off) {
  LHN_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && C % 16 == 0 && C <= 256 && save_off && scratch_off,
                "lhn_cbam_layout: N=%d H=%d W=%d C=%d (C a multiple of 16, <= 256)", N, H, W, C);
  const CbamLayout L = cbam_layout(N, H, W, C);
  const int64_t sv[10] = {L.avg, L.mx, L.amax, L.hid, L.g, L.s, L.cidx, L.a, L.ppart, L.save_total};
  const int64_t sc[8] = {L.dq, L.w7part, L.dgpart, L.davg, L.dmx, L.w1part, L.w2part, L.scratch_total};
  memcpy(save_off, sv, sizeof(sv));
  memcpy(scratch_off, sc, sizeof(sc));
  return 0;
}

static inline int cb_grid(int64_t items, int per_block) {
  int64_t nb = (items + per_block - 1) / per_block;
  const int64_t cap = (int64_t)lhn_num_cus() * 8;
  return (int)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

extern "C" int lhn_cbam_fwd(const lhn_view* p, const lhn_view* r, const float* w1, const float* w2, const float* w7,
                            const lhn_view* out, float* save, void* stream) {
  if (cbam_args_ok("lhn_cbam_fwd", p, r, out)) return 1;
  LHN_CHECK_ARG(w1 && w2 && w7 && save, "lhn_cbam_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int N = p->N, H = p->H, W = p->W, C = p->C, HW = H * W;
  const CbamLayout L = cbam_layout(N, H, W, C);
  const int64_t total = (int64_t)N * HW;
  float *avg = save + L.avg, *mx = save + L.mx, *hid = save + L.hid, *g = save + L.g, *sp = save + L.s, *a = save + L.a;
  int *amax = reinterpret_cast<int*>(save + L.amax), *cidx = reinterpret_cast<int*>(save + L.cidx);
  hipLaunchKernelGGL(k_cbam_pool, dim3(N * L.S), dim3(256), 0, s, *p, save + L.ppart, L.S);
  hipLaunchKernelGGL(k_cbam_mlp_fwd, dim3(N), dim3(256), 0, s, save + L.ppart, L.S, w1, w2, avg, mx, amax, hid, g, C, HW);
  const int C4 = C / 4;
#define CB_SPATIAL(LP) hipLaunchKernelGGL(k_cbam_spatial<LP>, dim3(cb_grid(total, 256 / LP)), dim3(256), 0, s, *p, g, sp, cidx, total)
  if (C4 <= 4) CB_SPATIAL(4);
  else if (C4 <= 8) CB_SPATIAL(8);
  else if (C4 <= 16) CB_SPATIAL(16);
  else if (C4 <= 32) CB_SPATIAL(32);
  else CB_SPATIAL(64);
#undef CB_SPATIAL
  hipLaunchKernelGGL(k_cbam_apply, dim3(L.ntx * L.nty, N), dim3(256), 0, s, *p, *r, *out, g, sp, w7, a, L.ntx);
  LHN_CHECK_LAUNCH("lhn_cbam_fwd");
  return 0;
}

extern "C" int lhn_cbam_bwd(const lhn_view* p, const lhn_view* r, const float* w1, const float* w2, const float* w7,
                            const lhn_view* out, const float* dout, float* dp, float* dr, float* dw1, float* dw2, float* dw7,
                            const float* save, float* scratch, void* stream) {
  if (cbam_args_ok("lhn_cbam_bwd", p, r, out)) return 1;
  LHN_CHECK_ARG(w1 && w2 && w7 && dout && dp && dr && dw1 && dw2 && dw7 && save && scratch, "lhn_cbam_bwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int N = p->N, H = p->H, W = p->W, C = p->C, HW = H * W, J = C / 16;
  const CbamLayout L = cbam_layout(N, H, W, C);
  const int64_t total = (int64_t)N * HW;
  const float *avg = save + L.avg, *mx = save + L.mx, *hid = save + L.hid, *g = save + L.g, *sp = save + L.s, *a = save + L.a;
  const int *amax = reinterpret_cast<const int*>(save + L.amax), *cidx = reinterpret_cast<const int*>(save + L.cidx);
  float *dq = scratch + L.dq, *w7part = scratch + L.w7part, *dgpart = scratch + L.dgpart, *davg = scratch + L.davg;
  float *dmx = scratch + L.dmx, *w1part = scratch + L.w1part, *w2part = scratch + L.w2part;
  const int C4 = C / 4, ntiles = L.ntx * L.nty;
#define CB_DQ(LP) \
  hipLaunchKernelGGL(k_cbam_dq<LP>, dim3(cb_grid(total, 256 / LP)), dim3(256), 0, s, *p, *out, dout, g, a, dq, dr, r->cstride, r->coff, total)
  if (C4 <= 4) CB_DQ(4);
  else if (C4 <= 8) CB_DQ(8);
  else if (C4 <= 16) CB_DQ(16);
  else if (C4 <= 32) CB_DQ(32);
  else CB_DQ(64);
#undef CB_DQ
  hipLaunchKernelGGL(k_cbam_du, dim3(ntiles, N), dim3(256), 0, s, *p, *out, dout, g, sp, a, cidx, dq, w7, dp, w7part, dgpart, L.ntx);
  hipLaunchKernelGGL(k_cbam_mlp_bwd, dim3(N), dim3(256), 0, s, dgpart, ntiles, w1, w2, avg, mx, hid, g, davg, dmx, w1part, w2part, C);
  hipLaunchKernelGGL(k_cbam_fold, dim3(1), dim3(256), 0, s, w7part, N * ntiles, 98, dw7);
  hipLaunchKernelGGL(k_cbam_fold, dim3((C * J + 255) / 256), dim3(256), 0, s, w1part, N, C * J, dw1);
  hipLaunchKernelGGL(k_cbam_fold, dim3((C * J + 255) / 256), dim3(256), 0, s, w2part, N, C * J, dw2);
  const int64_t total4 = total * C4;
  hipLaunchKernelGGL(k_cbam_dp, dim3(cb_grid(total4, 256)), dim3(256), 0, s, dp, p->cstride, p->coff, g, davg, dmx, amax, C, HW, total4);
  LHN_CHECK_LAUNCH("lhn_cbam_bwd");
  return 0;
}
