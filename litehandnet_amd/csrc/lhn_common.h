// Shared host/device helpers for liblhn (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include "../../include/lhn.h"

#define LHN_WAVE 64
// Elementwise kernels map thread -> (channel group c4 = tid % C4, pixel lane pl = tid / C4) with PL = 256 / C4 live lanes.
// C4 = C / 4 need not divide 256 (lite_hrnet.py: C = 20, 40, 80, 160, 320): the left-over threads (pl == PL) start their
// loops at LHN_DEAD, i.e. beyond any extent, and contribute zeros to reductions.
#define LHN_DEAD (1 << 30)
#define LHN_LANE0(pl, PL) ((pl) < (PL) ? (pl) : LHN_DEAD)

void lhn_set_error(const char* fmt, ...);

#define LHN_CHECK_ARG(cond, ...)                 \
  do {                                           \
    if (!(cond)) {                               \
      lhn_set_error(__VA_ARGS__);                \
      return 1;                                  \
    }                                            \
  } while (0)

#define LHN_CHECK_LAUNCH(name)                                                    \
  do {                                                                            \
    hipError_t e__ = hipGetLastError();                                           \
    if (e__ != hipSuccess) {                                                      \
      lhn_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));       \
      return 2;                                                                   \
    }                                                                             \
  } while (0)

// lhn_view.pend is reserved (round 2's deferred BatchNorm finalize, removed): every entry point wants NULL
static inline int lhn_no_pend(const lhn_view* v) { return !v || !v->pend; }

static inline int lhn_view_ok(const lhn_view* v) {
  return v && v->data && v->N > 0 && v->H > 0 && v->W > 0 && v->C > 0 && v->coff >= 0 &&
         v->coff + v->C <= v->cstride && (v->cstride % 4) == 0 && (v->coff % 4) == 0 && (v->C % 4) == 0;
}

// Host-side state is PER DEVICE (the library is re-entrant across devices: one process per GPU, or nn.DataParallel
// threads each bound to their own device, test.py:81): the CU count and every kernel's one-time attributes
// (hipFuncSetAttribute is a per-device setting) live in tables indexed by the calling thread's current device and are
// initialised under std::call_once.
#define LHN_MAX_DEVICES 16
static inline int lhn_device_slot() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0) d = 0;
  return d % LHN_MAX_DEVICES;
}
int lhn_num_cus();   // lhn_api.cpp: CUs of the current device; grid caps for persistent grid-stride kernels
bool lhn_deterministic_mode();   // LHN_DETERMINISTIC=1, see lhn_api.cpp
// grid of a persistent kernel: one block per `per_block` items, at most `cap_per_cu` blocks per CU
static inline int grid_for(int64_t items_per_block_total, int per_block, int cap_per_cu) {
  int64_t g = (items_per_block_total + per_block - 1) / per_block;
  const int64_t cap = (int64_t)lhn_num_cus() * cap_per_cu;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}
static inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// LHN_DW_GATHER=1 (read once per translation unit): the depthwise and stem convolutions run their row-gather kernels
// (k_conv_dw.hip, k_conv_stem.hip)
static inline bool lhn_dw_force_gather() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("LHN_DW_GATHER");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}
// The 1x1 convolution's cross-file functions.  pw_fwd_route / pw_bwd_route (k_conv_pw.hip) alone decide which a call reaches.
bool lhn_head_stream_on();      // LHN_HEAD_STREAM, as pw_switches() read it
// the shapes of the heatmap head's streaming kernels (k_conv_head.hip): 128 input channels, at most 32 features, whole weight
constexpr int HEAD_CIN = 128;
static inline bool lhn_head_shape(int Cin, int Cout, int wcols, int wrows) { return Cin == HEAD_CIN && Cout <= 32 && wcols == Cin && wrows == Cout; }
int lhn_head_fwd(const lhn_view* x, const float* w, const float* bias, float* y_nchw, int cout, int HoWo, int64_t bstride, hipStream_t s);
int lhn_head_bwd(const lhn_view* x, const float* w, const float* dy, float* dx, int dx_acc, float* dw, float* dbias, int cout, int HoWo,
                 int64_t bstride, int nrep, int64_t rep_stride, const lhn_gatesum* gs, hipStream_t s);
// Data gradient on the register-W forward kernel: dx[.., ci0 + n] (+)= sum_k dy[.., k] * W[co0 + k][ci0 + n].  dyv: the plain dy as a view
// of 32/64/128/256 output features, dxv: <= 128 input channels of the gradient buffer, w = &W[co0][ci0], wstride = the weight's Cin.
int lhn_pw_dgrad_wr(const lhn_view* dyv, const float* w, const lhn_view* dxv, int wstride, int accumulate, hipStream_t s);
// The three-launch backward (k_conv_kxk.hip).  dgrad: the kernel every output slice's data gradient takes
enum { LHN_PW_DGRAD_NONE = 0,      // dx is NULL
       LHN_PW_DGRAD_WR256,         // lhn_pw_dgrad_wr over all K = 256 output features at once
       LHN_PW_DGRAD_WR,            // lhn_pw_dgrad_wr per slice of <= 128 output features, later slices accumulating
       LHN_PW_DGRAD_KXK };         // k_kxk with one tap
int lhn_pw_bwd_split(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, float* dbias, int nrep, int64_t rep_stride, int dgrad, hipStream_t s);
// Its one-tap instances of k_kxk and k_kxk_wgrad: (K of the slice = output features / input channels, 32-wide tiles per block), the
// rest of the template arguments behind.  k_conv_kxk.hip instantiates exactly these; pw_split_route (k_conv_pw.hip) asks the predicate.
#define LHN_KXK_ONETAP(X, ...) \
  X(64, 4, __VA_ARGS__) X(128, 4, __VA_ARGS__) X(128, 2, __VA_ARGS__) X(64, 2, __VA_ARGS__) X(128, 1, __VA_ARGS__) X(32, 4, __VA_ARGS__)
static inline bool lhn_pw_split_instance(int k, int nt) {
#define LHN_X(K, NT, ...) || (k == K && nt == NT)
  return false LHN_KXK_ONETAP(LHN_X, 0);
#undef LHN_X
}
// Its tiles.  Slices are all alike (pw_split_route: channel counts above 128 are multiples of 128).  dgrad: 32 * ntd of the Cin
// features per block, nsplit blocks on gridDim.y, K = cc of the Cout channels per launch (LHN_PW_DGRAD_WR256: all 256 at once);
// wgrad: one launch per kc input channels (nk of them), 32 * nto output channels per block, cosplit groups on gridDim.z.
struct LhnPwSplitTiles {
  int ntd, nsplit, cc, nco;
  int nto, cosplit, kc, nk;
};
static inline LhnPwSplitTiles lhn_pw_split_tiles(int Cin, int Cout) {
  const int ntd = Cin >= 128 ? 4 : (Cin + 31) / 32, nto = Cout >= 128 ? 4 : (Cout + 31) / 32;
  return {ntd, (Cin + 32 * ntd - 1) / (32 * ntd), Cout < 128 ? Cout : 128, (Cout + 127) / 128,
          nto, (Cout + 32 * nto - 1) / (32 * nto), Cin < 128 ? Cin : 128, (Cin + 127) / 128};
}
// k_bottleneck.hip: lhn_bottleneck_fwd with the choice of skipping the tap-major copy of w2 (relayout = 0: wt_scratch holds it already)
int lhn_bottleneck_fwd_impl(const lhn_view* x, int Cm, const float* w1, const float* b1, const float* t1, const float* w2, const float* t2,
                            const float* w3, const float* b3, const float* t3, float out_slope, const lhn_view* y, float* wt_scratch,
                            int relayout, void* stream);
// k_stem.hip: lhn_stem_tail_fwd with the plan executor's choices -- tV is rows of a [3][tv_stride] table (the first m channels of the
// concatenation buffer's), relayout as above, check_slopes = 0 skips the blocking read-back of the tables' slope rows (the plan pass
// has looked at the slopes already, and a captured stream cannot be waited for)
int lhn_stem_tail_fwd_impl(const lhn_view* x, int K, const float* w_dw, const float* bT, const float* tT, const float* w1, const float* b1,
                           const float* tU, const float* w2, const float* b2, const float* tV, int tv_stride, const float* w3, const float* b3,
                           const lhn_view* y, float* wt_scratch, int relayout, int check_slopes, void* stream);

#ifdef __HIPCC__
// Workgroups of `kernel` (256 threads, `dyn_lds` bytes of dynamic LDS) that are resident on one CU at the same time: the
// occupancy API, never more than the LDS arithmetic with the kernel's static segment included (a persistent grid that
// over-estimates this by one runs a second, half-empty round -- measured: 3 x 54,784 B does not fit 160 KB).
template <typename F>
static inline int lhn_resident_per_cu(F kernel, size_t dyn_lds, int cap) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, dyn_lds) != hipSuccess || n < 1) n = 1;
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel)) == hipSuccess) {
    size_t per = (dyn_lds + a.sharedSizeBytes + 1023) / 1024 * 1024;
    const int by_lds = per ? (int)((160 * 1024) / per) : n;
    if (by_lds < n) n = by_lds;
  }
  if (n > cap) n = cap;
  return n < 1 ? 1 : n;
}

// One-time, per-device setup of a kernel: dynamic-LDS opt-in + resident workgroups per CU.  `static LhnKernelCfg cfg;`
// at the launch site (one per template instance); returns false when the LDS reservation is refused.
struct LhnKernelCfg {
  std::once_flag once[LHN_MAX_DEVICES];
  int per_cu[LHN_MAX_DEVICES];
  bool ok[LHN_MAX_DEVICES];
};
template <typename F>
static inline bool lhn_kernel_cfg(LhnKernelCfg& c, F kernel, size_t dyn_lds, int cap, int* per_cu) {
  const int d = lhn_device_slot();
  std::call_once(c.once[d], [&] {
    c.ok[d] = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)dyn_lds) == hipSuccess;
    c.per_cu[d] = lhn_resident_per_cu(kernel, dyn_lds, cap);
  });
  if (per_cu) *per_cu = c.per_cu[d];
  return c.ok[d];
}

// ---------------------------------------------------------------- device side
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float lhn_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }
// SiLU (models/pose_hg_ms_att.py:82,87): only the elementwise combine applies it (out_slope == LHN_SLOPE_SILU)
__device__ __forceinline__ float lhn_silu(float v) { return v / (1.f + expf(-v)); }
__device__ __forceinline__ float lhn_silu_grad(float v) {
  const float s = 1.f / (1.f + expf(-v));
  return s * (1.f + v * (1.f - s));
}

// pending transform of 4 consecutive channels of a view (absolute channel c, multiple of 4)
struct Xf4 {
  f4 sc, sh, sl;
};
__device__ __forceinline__ Xf4 lhn_load_xf(const lhn_view& v, int c_abs) {
  Xf4 t;
  if (v.table) {
    t.sc = *reinterpret_cast<const f4*>(v.table + c_abs);
    t.sh = *reinterpret_cast<const f4*>(v.table + v.cstride + c_abs);
    t.sl = *reinterpret_cast<const f4*>(v.table + 2 * v.cstride + c_abs);
  } else {
    t.sc = (f4){1.f, 1.f, 1.f, 1.f};
    t.sh = (f4){0.f, 0.f, 0.f, 0.f};
    t.sl = (f4){1.f, 1.f, 1.f, 1.f};
  }
  return t;
}
__device__ __forceinline__ f4 lhn_apply_xf(f4 raw, const Xf4& t) {
  f4 u = raw * t.sc + t.sh;
  f4 r;
  r.x = lhn_lrelu(u.x, t.sl.x);
  r.y = lhn_lrelu(u.y, t.sl.y);
  r.z = lhn_lrelu(u.z, t.sl.z);
  r.w = lhn_lrelu(u.w, t.sl.w);
  return r;
}
// consumed value of 4 channels at pixel index pix (= (n*H+h)*W+w), image n
__device__ __forceinline__ f4 lhn_load_val(const lhn_view& v, const Xf4& t, int64_t pix, int n, int c_abs) {
  f4 raw = *reinterpret_cast<const f4*>(v.data + pix * v.cstride + c_abs);
  f4 r = lhn_apply_xf(raw, t);
  if (v.gate) r *= *reinterpret_cast<const f4*>(v.gate + (int64_t)n * v.cstride + c_abs);
  return r;
}

// d(loss)/d(BN output u) and d(loss)/d(raw y) for 4 channels of a conv output, given the gradient
// w.r.t. the consumed value.  eff_dz = gate*dz + sum_bins dpool ;  du = eff_dz * lrelu'(u) ;
// dy = A*du + B*y + C  (coef == NULL: dy = du)
struct Gr4 {
  f4 A, B, Cc;
};
__device__ __forceinline__ Gr4 lhn_load_coef(const lhn_gradview& g, int cstride, int c_abs) {
  Gr4 r;
  if (g.coef) {
    r.A = *reinterpret_cast<const f4*>(g.coef + c_abs);
    r.B = *reinterpret_cast<const f4*>(g.coef + cstride + c_abs);
    r.Cc = *reinterpret_cast<const f4*>(g.coef + 2 * cstride + c_abs);
  } else {
    r.A = (f4){1.f, 1.f, 1.f, 1.f};
    r.B = (f4){0.f, 0.f, 0.f, 0.f};
    r.Cc = (f4){0.f, 0.f, 0.f, 0.f};
  }
  return r;
}
// adaptive-avg-pool(3x3) bin membership: bin i covers [floor(i*S/3), ceil((i+1)*S/3))
__device__ __forceinline__ int lhn_bin_lo(int i, int S) { return (i * S) / 3; }
__device__ __forceinline__ int lhn_bin_hi(int i, int S) { return ((i + 1) * S + 2) / 3; }

// The pooled gradient is stored per SEGMENT, not per bin: the three (possibly overlapping) bins cut each axis into at
// most five segments -- {bin0}, {bin0,bin1}, {bin1}, {bin1,bin2}, {bin2} -- and the attention backward writes
// dpool[n][sh*5+sw][c] = sum of (d loss / d pooled[bin]) / |bin| over the bins of segment (sh, sw).  A consumer then needs
// ONE branch-free load per pixel instead of a divergent loop over up to four bins.  H, W >= 2: on a 1-pixel axis the
// pixel lies in all three bins but reads the {bin1} segment only, so the writers' entry points refuse such a map.
#define LHN_DPOOL_SLOTS 25
__device__ __forceinline__ int lhn_pool_seg(int h, int S) {
  return (h >= lhn_bin_lo(1, S)) + (h >= lhn_bin_hi(0, S)) + (h >= lhn_bin_lo(2, S)) + (h >= lhn_bin_hi(1, S));
}
__device__ __forceinline__ f4 lhn_dpool_sum(const lhn_gradview& g, const lhn_view& v, int n, int h, int w, int c_abs) {
  const int slot = lhn_pool_seg(h, v.H) * 5 + lhn_pool_seg(w, v.W);
  return *reinterpret_cast<const f4*>(g.dpool + ((int64_t)n * LHN_DPOOL_SLOTS + slot) * v.cstride + c_abs);
}
// writer side: d[t] = d loss / d pooled[bin t] / |bin t| for the 9 bins of one (n, channel) -> the 25 segment sums
__device__ __forceinline__ void lhn_dpool_store(float* dpool, int64_t n, int cs, int c_abs, const float (&d)[9]) {
#pragma unroll
  for (int sh = 0; sh < 5; ++sh)
#pragma unroll
    for (int sw = 0; sw < 5; ++sw) {
      float v = 0.f;
#pragma unroll
      for (int bi = 0; bi < 3; ++bi)
#pragma unroll
        for (int bj = 0; bj < 3; ++bj) {
          const bool rin = (sh == 2 * bi) || (sh == 2 * bi - 1) || (sh == 2 * bi + 1);
          const bool cin = (sw == 2 * bj) || (sw == 2 * bj - 1) || (sw == 2 * bj + 1);
          if (rin && cin) v += d[bi * 3 + bj];
        }
      dpool[(n * LHN_DPOOL_SLOTS + sh * 5 + sw) * cs + c_abs] = v;
    }
}
// returns du (gradient at the BN output) and, through *val_out, nothing else; raw = y
__device__ __forceinline__ f4 lhn_grad_du(const lhn_view& v, const lhn_gradview& g, const Xf4& t, f4 raw, f4 dz,
                                          int n, int h, int w, int c_abs) {
  f4 e = dz;
  if (v.gate) e *= *reinterpret_cast<const f4*>(v.gate + (int64_t)n * v.cstride + c_abs);
  f4 u = raw * t.sc + t.sh;
  f4 du;
  du.x = e.x * (u.x > 0.f ? 1.f : t.sl.x);
  du.y = e.y * (u.y > 0.f ? 1.f : t.sl.y);
  du.z = e.z * (u.z > 0.f ? 1.f : t.sl.z);
  du.w = e.w * (u.w > 0.f ? 1.f : t.sl.w);
  if (g.dpool) {
    f4 dp = lhn_dpool_sum(g, v, n, h, w, c_abs);   // pooled value is the *post-activation* value
    du.x += dp.x * (u.x > 0.f ? 1.f : t.sl.x);
    du.y += dp.y * (u.y > 0.f ? 1.f : t.sl.y);
    du.z += dp.z * (u.z > 0.f ? 1.f : t.sl.z);
    du.w += dp.w * (u.w > 0.f ? 1.f : t.sl.w);
  }
  return du;
}

// Lean dy for the MFMA loaders: gate (1 if none) is passed in, the channel-attention pooled gradient is
// handled by the caller on a separate (rare) path.
__device__ __forceinline__ f4 lhn_dy_fast(const Xf4& t, const Gr4& gr, f4 raw, f4 dz, f4 gate) {
  const f4 u = raw * t.sc + t.sh;
  const f4 dl = (f4){u.x > 0.f ? 1.f : t.sl.x, u.y > 0.f ? 1.f : t.sl.y, u.z > 0.f ? 1.f : t.sl.z, u.w > 0.f ? 1.f : t.sl.w};
  return gr.A * (dz * gate * dl) + gr.B * raw + gr.Cc;
}

// ---- last-block-arrives hand-off for ATOMIC accumulators.  The only bytes handed over are sums built with
// device-scope atomic adds, which execute at the memory side and never sit in an L1/L2 (MI355X_MICROARCH
// "Global float atomics"), so no cache write-back / invalidate is needed (a release fence here costs a
// buffer_wbl2 per workgroup and made every conv slower than the separate finalize launch it replaced):
// each wave waits until its own atomics are acknowledged (vmcnt(0)), the block meets at a barrier, ONE lane
// takes a ticket with a device-scope atomic; the block that draws the last ticket reads the sums with
// device-scope (sc1, L1-bypassing) loads.  Nothing else in the launch ever reads those addresses.
// Tickets in TWO levels (counter[0] = top, counter[1 + g] = group g = block % 32): returning atomics on ONE word are served at
// ~88 per us, so 1,024 workgroups finishing together queued 12 us on a single word (round 1: fused finalize slower than the
// launch it replaced); 32 group words take their tickets in parallel, the last of each group takes one of 32 top tickets.
#define LHN_TICKET_WORDS 33
__device__ __forceinline__ bool lhn_last_block(unsigned* counter) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned nb = gridDim.x * gridDim.y, b = blockIdx.x + blockIdx.y * gridDim.x;
    const unsigned g = b & 31u, ng = nb < 32u ? nb : 32u, gsize = (nb - g + 31u) >> 5;
    int last = 0;
    if (__hip_atomic_fetch_add(counter + 1 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gsize - 1u)
      last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ng - 1u;
    s_last = last;
  }
  __syncthreads();
  return s_last != 0;
}
__device__ __forceinline__ double lhn_ld_agent(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// train-mode BatchNorm finalize by one whole block (same arithmetic as k_bn_finalize)
__device__ __forceinline__ void lhn_bn_finalize_block(const lhn_bnfin& f, const double* stats) {
  const int C = f.C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double s1 = 0, s2 = 0;
    for (int r = 0; r < LHN_STAT_REPLICAS; ++r) {
      s1 += lhn_ld_agent(stats + (size_t)r * 2 * C + c);
      s2 += lhn_ld_agent(stats + (size_t)r * 2 * C + C + c);
    }
    const double mean = s1 / f.count;
    double var = s2 / f.count - mean * mean;
    if (var < 0) var = 0;
    if (f.running_mean) {
      const double bm = mean + (f.conv_bias ? (double)f.conv_bias[c] : 0.0);
      f.running_mean[c] = (float)((1.0 - (double)f.momentum) * (double)f.running_mean[c] + (double)f.momentum * bm);
      const double unb = f.count > 1 ? var * f.count / (f.count - 1.0) : var;
      f.running_var[c] = (float)((1.0 - (double)f.momentum) * (double)f.running_var[c] + (double)f.momentum * unb);
    }
    const float invstd = (float)(1.0 / sqrt(var + (double)f.eps));
    const float g = f.gamma ? f.gamma[c] : 1.f, b = f.beta ? f.beta[c] : 0.f;
    const float sc = g * invstd;
    f.table[f.coff + c] = sc;
    f.table[f.cstride + f.coff + c] = b - (float)mean * sc;
    f.table[2 * f.cstride + f.coff + c] = f.slope;
    if (f.save_mean_invstd) {
      f.save_mean_invstd[c] = (float)mean;
      f.save_mean_invstd[C + c] = invstd;
    }
  }
  if (f.num_batches_tracked && threadIdx.x == 0) f.num_batches_tracked[0] += 1;
}
// the same by a whole block with the replica fold spread over its threads (blockDim.x / C groups of replicas per channel meet in
// `part`, LDS for 2 * blockDim.x doubles that nobody else is using any more): one memory latency instead of 64 dependent loads
__device__ __forceinline__ void lhn_bn_finalize_block_par(const lhn_bnfin& f, const double* stats, double* part) {
  const int C = f.C, nt = blockDim.x, tid = threadIdx.x;
  int G = nt / C;
  G = G < 1 ? 1 : (G > LHN_STAT_REPLICAS ? LHN_STAT_REPLICAS : G);
  __syncthreads();      // (part may alias LDS the block was still reading)
  for (int c0 = 0; c0 < C; c0 += nt) {
    const int g = G > 1 ? tid / C : 0, c = c0 + (G > 1 ? tid - g * C : tid);
    if (c0) __syncthreads();
    if (g < G && c < C) {
      double s1 = 0, s2 = 0;
#pragma unroll 4
      for (int r = g; r < LHN_STAT_REPLICAS; r += G) {
        s1 += lhn_ld_agent(stats + (size_t)r * 2 * C + c);
        s2 += lhn_ld_agent(stats + (size_t)r * 2 * C + C + c);
      }
      part[2 * tid] = s1;
      part[2 * tid + 1] = s2;
    }
    __syncthreads();
    if (g != 0 || c >= C) continue;
    double s1 = 0, s2 = 0;
    for (int k = 0; k < G; ++k) {
      s1 += part[2 * (k * C + tid)];
      s2 += part[2 * (k * C + tid) + 1];
    }
    const double mean = s1 / f.count;
    double var = s2 / f.count - mean * mean;
    if (var < 0) var = 0;
    if (f.running_mean) {
      const double bm = mean + (f.conv_bias ? (double)f.conv_bias[c] : 0.0);
      f.running_mean[c] = (float)((1.0 - (double)f.momentum) * (double)f.running_mean[c] + (double)f.momentum * bm);
      const double unb = f.count > 1 ? var * f.count / (f.count - 1.0) : var;
      f.running_var[c] = (float)((1.0 - (double)f.momentum) * (double)f.running_var[c] + (double)f.momentum * unb);
    }
    const float invstd = (float)(1.0 / sqrt(var + (double)f.eps));
    const float gm = f.gamma ? f.gamma[c] : 1.f, b = f.beta ? f.beta[c] : 0.f;
    const float sc = gm * invstd;
    f.table[f.coff + c] = sc;
    f.table[f.cstride + f.coff + c] = b - (float)mean * sc;
    f.table[2 * f.cstride + f.coff + c] = f.slope;
    if (f.save_mean_invstd) {
      f.save_mean_invstd[c] = (float)mean;
      f.save_mean_invstd[C + c] = invstd;
    }
  }
  if (f.num_batches_tracked && tid == 0) f.num_batches_tracked[0] += 1;
}
__device__ __forceinline__ void lhn_bn_bwd_finalize_block(const lhn_bnbwdfin& f, const double* sums, const float* save) {
  const int C = f.C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double db = 0, dg = 0;
    for (int r = 0; r < LHN_STAT_REPLICAS; ++r) {
      db += lhn_ld_agent(sums + (size_t)r * 2 * C + c);
      dg += lhn_ld_agent(sums + (size_t)r * 2 * C + C + c);
    }
    const double mean = save[c], inv = save[C + c], s = (double)(f.gamma ? f.gamma[c] : 1.f) * inv;
    f.coef[f.coff + c] = (float)s;
    f.coef[f.cstride + f.coff + c] = (float)(-s * inv * dg / f.count);
    f.coef[2 * f.cstride + f.coff + c] = (float)(-s * db / f.count + s * inv * mean * dg / f.count);
    if (f.dgamma) f.dgamma[c] += (float)dg;
    if (f.dbeta) f.dbeta[c] += (float)db;
  }
}
// ---- BatchNorm-backward finalize, shared by k_bn_bwd_finalize and the prologues of the convolution backward kernels that fold
// their own channels (lhn_bnbwdsrc).  Replica order of the separate launch: G = clamp(LHN_FIN_THREADS / C_bn, 1, 32) groups, group
// g adds replicas g, g + G, ... in turn, the groups are then added in the order 0 .. G-1; plain loads (the sums were completed by
// an earlier launch).  Same sums in memory, same bits out, whoever calls.
#define LHN_FIN_THREADS 1024
__device__ __forceinline__ int lhn_fin_groups(int C_bn) {
  const int G = LHN_FIN_THREADS / C_bn;
  return G < 1 ? 1 : (G > LHN_STAT_REPLICAS ? LHN_STAT_REPLICAS : G);
}
// first half: the group partials of channels [c0, c0 + nc) into part[2 * (g * nc + cl)] (sum du), [.. + 1] (sum du * xhat);
// part = 2 * G * nc doubles of LDS.  A barrier separates it from lhn_bn_bwd_coef.
__device__ __forceinline__ void lhn_bn_bwd_fold_part(const double* __restrict__ sums, int SC, int c0, int nc, int G, double* part) {
  for (int i = threadIdx.x; i < G * nc; i += blockDim.x) {
    const int g = i / nc, c = c0 + (i - g * nc);
    double s1 = 0, s2 = 0;
#pragma unroll 4
    for (int r = g; r < LHN_STAT_REPLICAS; r += G) {
      s1 += sums[(size_t)r * 2 * SC + c];
      s2 += sums[(size_t)r * 2 * SC + SC + c];
    }
    part[2 * i] = s1;
    part[2 * i + 1] = s2;
  }
}
// second half, one thread per channel cl of the nc: dy = A*du + B*y + C with  A = s, B = -s*invstd*dgamma/n,
// C = -s*dbeta/n + s*invstd*mean*dgamma/n, s = gamma*invstd
struct LhnBwdCoef {
  float A, B, C;
  double db, dg;      // sum du, sum du * xhat
};
__device__ __forceinline__ LhnBwdCoef lhn_bn_bwd_coef_of(double db, double dg, float gamma, float save_mean, float save_invstd, double count) {
  LhnBwdCoef r;
  const double mean = save_mean, inv = save_invstd, s = (double)gamma * inv;
  r.A = (float)s;
  r.B = (float)(-s * inv * dg / count);
  r.C = (float)(-s * db / count + s * inv * mean * dg / count);
  r.db = db;
  r.dg = dg;
  return r;
}
__device__ __forceinline__ LhnBwdCoef lhn_bn_bwd_coef(const double* part, int nc, int G, int cl, float gamma, float save_mean,
                                                      float save_invstd, double count) {
  double db = 0, dg = 0;
  for (int k = 0; k < G; ++k) {
    db += part[2 * (k * nc + cl)];
    dg += part[2 * (k * nc + cl) + 1];
  }
  return lhn_bn_bwd_coef_of(db, dg, gamma, save_mean, save_invstd, count);
}
// what the finalize leaves in memory for BatchNorm channel c (coef at absolute channel coff + c of a [3][cs] table)
__device__ __forceinline__ void lhn_bn_bwd_coef_store(const LhnBwdCoef& r, float* __restrict__ coef, int cs, int coff, int c,
                                                      float* __restrict__ dgamma, float* __restrict__ dbeta, float pgrad_scale) {
  coef[coff + c] = r.A;
  coef[cs + coff + c] = r.B;
  coef[2 * cs + coff + c] = r.C;
  if (dgamma) dgamma[c] += (float)r.dg * pgrad_scale;
  if (dbeta) dbeta[c] += (float)r.db * pgrad_scale;
}
// ---- the same inside a convolution backward prologue (256 threads, channels [c0, c0 + nc) of the BatchNorm of y).  A prologue is
// memory latency end to end, so each thread issues ALL of its loads -- its share of the sums, and the gamma / mean / invstd of the
// channel it finishes -- before the first add: one latency, where a loop over entries pays one per trip.
struct LhnBwdPre {
  float gamma, mean, inv;
};
__device__ __forceinline__ LhnBwdPre lhn_bn_bwd_pre(const lhn_bnbwdsrc& f, int c0, int nc) {
  LhnBwdPre p;
  const int c = c0 + min((int)threadIdx.x, nc - 1);
  p.gamma = f.gamma ? f.gamma[c] : 1.f;
  p.mean = f.save_mean_invstd[c];
  p.inv = f.save_mean_invstd[f.stat_channels + c];
  return p;
}
// first half, G and NC known at compile time with G * NC = 1,024 entries (the register-W 1x1: NC = COUT): group partials as
// lhn_bn_bwd_fold_part leaves them, 32 * NC / 128 loads per thread in flight together
template <int NC>
__device__ __forceinline__ void lhn_bn_bwd_fold_part_ct(const double* __restrict__ sums, int SC, double* part) {
  constexpr int G = LHN_FIN_THREADS / NC, NE = 4, NR = LHN_STAT_REPLICAS / G;
  static_assert(G * NC == LHN_FIN_THREADS && G <= LHN_STAT_REPLICAS && G * NR == LHN_STAT_REPLICAS, "NC in {32, 64, 128}");
  double a[NE][NR], b[NE][NR];
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const int i = threadIdx.x + 256 * j, g = i / NC, c = i % NC;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      a[j][k] = sums[(size_t)(g + k * G) * 2 * SC + c];
      b[j][k] = sums[(size_t)(g + k * G) * 2 * SC + SC + c];
    }
  }
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    double s1 = 0, s2 = 0;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      s1 += a[j][k];
      s2 += b[j][k];
    }
    part[2 * (threadIdx.x + 256 * j)] = s1;
    part[2 * (threadIdx.x + 256 * j) + 1] = s2;
  }
}
// first half for nc <= 32 channels and any C_bn (the depthwise rows kernel): the 32 * nc (sum du, sum du * xhat) pairs go to LDS as
// they are, raw[2 * (r * nc + cl)] (512 * nc bytes), at most 4 pairs per thread
__device__ __forceinline__ void lhn_bn_bwd_fold_raw(const double* __restrict__ sums, int SC, int c0, int nc, double* raw) {
  double a[4], b[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = min((int)threadIdx.x + 256 * q, LHN_STAT_REPLICAS * nc - 1), r = p / nc, cl = p - r * nc;
    a[q] = sums[(size_t)r * 2 * SC + c0 + cl];
    b[q] = sums[(size_t)r * 2 * SC + SC + c0 + cl];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = threadIdx.x + 256 * q;
    if (p < LHN_STAT_REPLICAS * nc) {
      raw[2 * p] = a[q];
      raw[2 * p + 1] = b[q];
    }
  }
}
// ... and its second half: thread cl adds the replicas of its channel in the finalize's order (groups of C_bn, then the groups)
__device__ __forceinline__ LhnBwdCoef lhn_bn_bwd_coef_raw(const double* raw, int nc, int G, int cl, const LhnBwdPre& p, double count) {
  double db = 0, dg = 0;
  for (int g = 0; g < G; ++g) {
    double s1 = 0, s2 = 0;
    for (int r = g; r < LHN_STAT_REPLICAS; r += G) {
      s1 += raw[2 * (r * nc + cl)];
      s2 += raw[2 * (r * nc + cl) + 1];
    }
    db += s1;
    dg += s2;
  }
  return lhn_bn_bwd_coef_of(db, dg, p.gamma, p.mean, p.inv, count);
}
// the LDS slots A | B | C of channel cl (cfA[cl], cfA[ld + cl], cfA[2 * ld + cl]); `lead` (block-uniform): this workgroup also
// writes memory.  No barrier here: the caller's next one publishes the slots (and frees the fold's scratch).
__device__ __forceinline__ void lhn_bn_bwd_coef_put(const LhnBwdCoef& r, const lhn_bnbwdsrc& f, float* __restrict__ coef, int cs, int coff,
                                                    int c, float* cfA, int ld, int cl, bool lead) {
  cfA[cl] = r.A;
  cfA[ld + cl] = r.B;
  cfA[2 * ld + cl] = r.C;
  if (lead) lhn_bn_bwd_coef_store(r, coef, cs, coff, c, f.dgamma, f.dbeta, f.pgrad_scale);
}
// ---- BatchNorm FORWARD finalize, shared by k_bn_finalize and the prologues of the forward kernels that fold their own input
// channels (lhn_bnfinsrc).  Replica order of the separate launch: G = lhn_fin_groups(C_bn) groups, group g adds replicas g, g + G, ...
// in turn, the groups are then added in the order 0 .. G-1.  Same sums in memory, same bits out, whoever calls.
// the arithmetic of one channel: batch moments from the folded sums ...
__device__ __forceinline__ void lhn_bn_fin_moments(double s1, double s2, double count, double& mean, double& var) {
  mean = s1 / count;
  var = s2 / count - mean * mean;
  if (var < 0) var = 0;
}
// ... one momentum step of the running statistics (cb: bias of the convolution in front, which the stored output excludes) ...
__device__ __forceinline__ void lhn_bn_fin_running(float* __restrict__ rmean, float* __restrict__ rvar, int c, float rm, float rv,
                                                   double mean, double var, double cb, double count, float momentum) {
  rmean[c] = (float)((1.0 - (double)momentum) * (double)rm + (double)momentum * (mean + cb));
  const double unb = count > 1 ? var * count / (count - 1.0) : var;
  rvar[c] = (float)((1.0 - (double)momentum) * (double)rv + (double)momentum * unb);
}
// ... and the table entry
struct LhnFinTab {
  float sc, sh, invstd;
};
__device__ __forceinline__ LhnFinTab lhn_bn_fin_tab(double mean, double var, float eps, float gm, float b) {
  LhnFinTab r;
  r.invstd = (float)(1.0 / sqrt(var + (double)eps));
  r.sc = gm * r.invstd;
  r.sh = b - (float)mean * r.sc;
  return r;
}
// Prologue form (256 threads, channels [c0, c0 + nc) of the BatchNorm of x, nc * 32 <= 256 * Q).  As in the backward prologues each
// thread issues ALL of its loads -- its share of the statistics, and the parameters of the channel it finishes -- before the first
// add, and IN FRONT of the first tile's loads: loads return in order, so a fold whose loads stand behind the tile's would wait for
// the whole tile and run after it instead of under it (measured: 4 us per launch against 5.3 us for the launch it replaces).
// lead (block-uniform): this workgroup also writes memory.
struct LhnFinPre {
  float gamma, beta, cb, rm, rv;
};
__device__ __forceinline__ LhnFinPre lhn_bn_fin_pre(const lhn_bnfinsrc& f, int c0, int nc, bool lead) {
  LhnFinPre p;
  const int c = c0 + min((int)threadIdx.x, nc - 1);
  p.gamma = f.gamma ? f.gamma[c] : 1.f;
  p.beta = f.beta ? f.beta[c] : 0.f;
  p.cb = (lead && f.conv_bias) ? f.conv_bias[c] : 0.f;
  p.rm = (lead && f.running_mean) ? f.running_mean[c] : 0.f;
  p.rv = (lead && f.running_mean) ? f.running_var[c] : 0.f;
  return p;
}
// first half: the 32 * nc (sum, sum of squares) pairs, Q per thread, into registers (in front of the tile's loads) ...
template <int Q>
__device__ __forceinline__ void lhn_bn_fin_load(const double* __restrict__ stats, int SC, int c0, int nc, double (&a)[Q], double (&b)[Q]) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int p = min((int)threadIdx.x + 256 * q, LHN_STAT_REPLICAS * nc - 1), r = p / nc, cl = p - r * nc;
    a[q] = stats[(size_t)r * 2 * SC + c0 + cl];
    b[q] = stats[(size_t)r * 2 * SC + SC + c0 + cl];
  }
}
// ... and to LDS as they are (behind them), raw[2 * (r * nc + cl)] (512 * nc bytes)
template <int Q>
__device__ __forceinline__ void lhn_bn_fin_put(const double (&a)[Q], const double (&b)[Q], int nc, double* raw) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int p = threadIdx.x + 256 * q;
    if (p < LHN_STAT_REPLICAS * nc) {
      raw[2 * p] = a[q];
      raw[2 * p + 1] = b[q];
    }
  }
}
// second half (behind a barrier), thread cl < nc: the replicas of its channel added in the finalize's order (groups of G, then the
// groups).  GC = G at compile time (a divisor of 32), 0 = any G: with GC the 32 LDS reads are one batch in flight, where the loop
// over a run-time G pays one LDS latency per replica (a microsecond of the prologue at G = 32)
template <int GC>
__device__ __forceinline__ void lhn_bn_fin_sum(const double* raw, int nc, int cl, int G, double& s1, double& s2) {
  s1 = 0;
  s2 = 0;
  if constexpr (GC > 0) {
    static_assert(LHN_STAT_REPLICAS % GC == 0, "whole groups");
    const double* rc = raw + 2 * cl;
#pragma unroll
    for (int g = 0; g < GC; ++g) {
      double t1 = 0, t2 = 0;
#pragma unroll
      for (int r = g; r < LHN_STAT_REPLICAS; r += GC) {
        t1 += rc[2 * r * nc];
        t2 += rc[2 * r * nc + 1];
      }
      s1 += t1;
      s2 += t2;
    }
  } else {
    for (int g = 0; g < G; ++g) {
      double t1 = 0, t2 = 0;
      for (int r = g; r < LHN_STAT_REPLICAS; r += G) {
        t1 += raw[2 * (r * nc + cl)];
        t2 += raw[2 * (r * nc + cl) + 1];
      }
      s1 += t1;
      s2 += t2;
    }
  }
}
// the G of a workgroup's BatchNorm at run time: the two values the models' depthwise chains have (C = 32: 32, C = 64: 16) take the
// compile-time form
__device__ __forceinline__ void lhn_bn_fin_sum_any(const double* raw, int nc, int cl, int C_bn, double& s1, double& s2) {
  const int G = lhn_fin_groups(C_bn);
  if (G == 32) lhn_bn_fin_sum<32>(raw, nc, cl, G, s1, s2);
  else if (G == 16) lhn_bn_fin_sum<16>(raw, nc, cl, G, s1, s2);
  else lhn_bn_fin_sum<0>(raw, nc, cl, G, s1, s2);
}
// ... and the channel's table entry into the LDS slots tab[cl] | tab[ld + cl] | tab[2 * ld + cl] (scale | shift | slope); the lead
// workgroup stores what lhn_bn_finalize leaves in memory.  No barrier here: the caller's next one publishes the slots and frees raw.
__device__ __forceinline__ void lhn_bn_fin_channel(const lhn_bnfinsrc& f, const LhnFinPre& p, double s1, double s2, int c0, int cl,
                                                   bool lead, float* tab, int ld) {
  const int c = c0 + cl;
  double mean, var;
  lhn_bn_fin_moments(s1, s2, f.count, mean, var);
  const LhnFinTab t = lhn_bn_fin_tab(mean, var, f.eps, p.gamma, p.beta);
  tab[cl] = t.sc;
  tab[ld + cl] = t.sh;
  tab[2 * ld + cl] = f.slope;
  if (lead) {
    if (f.running_mean) lhn_bn_fin_running(f.running_mean, f.running_var, c, p.rm, p.rv, mean, var, (double)p.cb, f.count, f.momentum);
    f.table[f.coff + c] = t.sc;
    f.table[f.cstride + f.coff + c] = t.sh;
    f.table[2 * f.cstride + f.coff + c] = f.slope;
    if (f.save_mean_invstd) {
      f.save_mean_invstd[c] = (float)mean;
      f.save_mean_invstd[f.C + c] = t.invstd;
    }
    if (c == 0 && f.num_batches_tracked) f.num_batches_tracked[0] += 1;
  }
}
__device__ __forceinline__ Xf4 lhn_bn_fin_xf(const float* tab, int ld, int cl4) {
  Xf4 t;
  t.sc = *reinterpret_cast<const f4*>(tab + cl4);
  t.sh = *reinterpret_cast<const f4*>(tab + ld + cl4);
  t.sl = *reinterpret_cast<const f4*>(tab + 2 * ld + cl4);
  return t;
}
static __device__ __forceinline__ lhn_bnfin lhn_nofin() {
  lhn_bnfin f;
  f.counter = nullptr;
  return f;
}

// Block-wide per-channel sums for the thread layout (c4 = tid % C4 float4 channel groups, pixel lane = tid / C4) with
// C4 in {8, 16, 32}: lanes of a wave that share c4 meet by xor-shuffles, the four waves through `red` (>= 8*C4 float4 of
// LDS that nobody else is using), then 8*C4 threads add one double each into st0[4*c4+j] (sums) / st1[4*c4+j] (second sums).
// Replaces a C4-thread serial loop over 256/C4 LDS rows that cost 4-10 us per launch.
__device__ __forceinline__ void lhn_block_stat_atomics(f4 s, f4 q, int C4, f4* red, double* st0, double* st1, int nvalid = 64) {
  for (int o = C4; o < 64; o <<= 1) {
    s.x += __shfl_xor(s.x, o, 64); s.y += __shfl_xor(s.y, o, 64); s.z += __shfl_xor(s.z, o, 64); s.w += __shfl_xor(s.w, o, 64);
    q.x += __shfl_xor(q.x, o, 64); q.y += __shfl_xor(q.y, o, 64); q.z += __shfl_xor(q.z, o, 64); q.w += __shfl_xor(q.w, o, 64);
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  if (lane < C4) {
    red[(wave * C4 + lane) * 2] = s;
    red[(wave * C4 + lane) * 2 + 1] = q;
  }
  __syncthreads();
  if (tid < 8 * C4) {
    const int kind = tid / (4 * C4), r = tid - kind * 4 * C4, cc = r >> 2, jj = r & 3;
    double v = 0;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) {
      const f4 a = red[(wv * C4 + cc) * 2 + kind];
      v += (double)(jj == 0 ? a.x : jj == 1 ? a.y : jj == 2 ? a.z : a.w);
    }
    if (cc < nvalid) atomicAdd((kind ? st1 : st0) + 4 * cc + jj, v);      // nvalid: channel groups that exist (tail of C % 32)
  }
}

// lhn_load_xf from an explicit table pointer; tab == NULL = identity
__device__ __forceinline__ Xf4 lhn_load_xf_t(const float* tab, int cstride, int c_abs) {
  Xf4 t;
  if (tab) {
    t.sc = *reinterpret_cast<const f4*>(tab + c_abs);
    t.sh = *reinterpret_cast<const f4*>(tab + cstride + c_abs);
    t.sl = *reinterpret_cast<const f4*>(tab + 2 * cstride + c_abs);
  } else {
    t.sc = (f4){1.f, 1.f, 1.f, 1.f};
    t.sh = (f4){0.f, 0.f, 0.f, 0.f};
    t.sl = (f4){1.f, 1.f, 1.f, 1.f};
  }
  return t;
}

// Per-tile BatchNorm partial sums, SHIFTED: within one tile a thread accumulates sum(v - K) and sum((v - K)^2) in fp32 with
// K = the first value it saw in this tile (differences of the order of sigma: no cancellation, full fp32 relative accuracy
// even when |mean| = 1000 sigma), and un-shifts in double when the tile is done:
//   sum v   = s + n K            sum v^2 = q + 2 K s + n K^2
struct TileStat {
  float k, s, q;
  int n;
  __device__ __forceinline__ void reset() { n = 0; k = s = q = 0.f; }
  __device__ __forceinline__ void add(float v) {
    if (n == 0) k = v;
    const float d = v - k;
    s += d;
    q += d * d;
    ++n;
  }
  __device__ __forceinline__ void flush(double& sum, double& sq) const {
    const double K = (double)k, S = (double)s;
    sum += S + (double)n * K;
    sq += (double)q + 2.0 * K * S + (double)n * K * K;
  }
};

// float4 form: sd / qd (double[4]) += the un-shifted sums of n values accumulated as s = sum(v - k), q = sum((v - k)^2)
__device__ __forceinline__ void lhn_unshift4(double (&sd)[4], double (&qd)[4], f4 s, f4 q, f4 k, int n) {
  const float sv[4] = {s.x, s.y, s.z, s.w}, qv[4] = {q.x, q.y, q.z, q.w}, kv[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double K = (double)kv[j], S = (double)sv[j];
    sd[j] += S + (double)n * K;
    qd[j] += (double)qv[j] + 2.0 * K * S + (double)n * K * K;
  }
}

// The same reduction for DOUBLE per-thread sums (convolution epilogues promote their per-tile fp32 partials to double: a
// running fp32 sum of squares over thousands of pixels loses the variance when |mean| >> sigma).  red: >= 32*C4 doubles.
__device__ __forceinline__ void lhn_block_stat_atomics_d(const double (&s)[4], const double (&q)[4], int C4, double* red,
                                                         double* st0, double* st1, int nvalid = 64) {
  double v[8] = {s[0], s[1], s[2], s[3], q[0], q[1], q[2], q[3]};
  for (int o = C4; o < 64; o <<= 1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += __shfl_xor(v[i], o, 64);
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  if (lane < C4) {
#pragma unroll
    for (int i = 0; i < 8; ++i) red[(wave * C4 + lane) * 8 + i] = v[i];
  }
  __syncthreads();
  if (tid < 8 * C4) {
    const int kind = tid / (4 * C4), r = tid - kind * 4 * C4, cc = r >> 2, jj = r & 3;
    double t = 0;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) t += red[(wv * C4 + cc) * 8 + kind * 4 + jj];
    if (cc < nvalid) atomicAdd((kind ? st1 : st0) + 4 * cc + jj, t);
  }
}

// ---- reader-side BatchNorm-backward sums (lhn_bnsum), elementwise thread layout (c4 = tid % C4 float4 channel groups of the
// reader's input view, pixel lane = tid / C4; dead lanes carry zeros): block reduction + one double atomic per channel and
// block into the producer's replica (blockIdx.x % LHN_STAT_REPLICAS).  red: >= 512 float4 of LDS nobody else is using.
__device__ __forceinline__ void lhn_bns_flush(const lhn_bnsum& b, f4 s, f4 q, int C4, f4* red) {
  double* st = b.sums + (size_t)(blockIdx.x % LHN_STAT_REPLICAS) * 2 * b.C + b.coff;
  if (C4 <= 32 && (C4 & (C4 - 1)) == 0) {
    lhn_block_stat_atomics(s, q, C4, red, st, st + b.C);
  } else {
    const int PL = 256 / C4;
    __syncthreads();
    red[threadIdx.x * 2] = s;
    red[threadIdx.x * 2 + 1] = q;
    __syncthreads();
    if ((int)threadIdx.x < C4) {
      double sd[4] = {0, 0, 0, 0}, qd[4] = {0, 0, 0, 0};
      for (int j = 0; j < PL; ++j) {
        const f4 a = red[(j * C4 + threadIdx.x) * 2], c = red[(j * C4 + threadIdx.x) * 2 + 1];
        sd[0] += a.x; sd[1] += a.y; sd[2] += a.z; sd[3] += a.w;
        qd[0] += c.x; qd[1] += c.y; qd[2] += c.z; qd[3] += c.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        atomicAdd(st + 4 * threadIdx.x + j, sd[j]);
        atomicAdd(st + b.C + 4 * threadIdx.x + j, qd[j]);
      }
    }
  }
}
// derivative of the pending activation at the raw value
__device__ __forceinline__ f4 lhn_dact_xf(f4 raw, const Xf4& t) {
  const f4 u = raw * t.sc + t.sh;
  return (f4){u.x > 0.f ? 1.f : t.sl.x, u.y > 0.f ? 1.f : t.sl.y, u.z > 0.f ? 1.f : t.sl.z, u.w > 0.f ? 1.f : t.sl.w};
}

__device__ __forceinline__ float lhn_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double lhn_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
#endif
