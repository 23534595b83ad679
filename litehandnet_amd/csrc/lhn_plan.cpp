// Static plan executor: one call enqueues a whole forward or backward pass on a HIP stream.
// The plan (buffers + op lists) is produced by the Python mirror of the reference's module tree;
// this file only resolves offsets into the workspace arena / parameter array and calls the launchers.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "lhn_common.h"

// reader-side BatchNorm sums (lhn_bnsum) of an op: byte offsets of the producer's sums / saved statistics, channels, offset
static lhn_bnsum mkbns(void* ws, int64_t sums_off, int64_t save_off, int C, int coff) {
  lhn_bnsum b;
  memset(&b, 0, sizeof(b));
  if (sums_off >= 0 && save_off >= 0 && C > 0) {
    b.sums = reinterpret_cast<double*>(static_cast<char*>(ws) + sums_off);
    b.save = reinterpret_cast<const float*>(static_cast<char*>(ws) + save_off);
    b.C = C;
    b.coff = coff;
  }
  return b;
}

enum {
  OP_STEM = 1, OP_PW = 2, OP_DW = 3, OP_KXK = 4, OP_FINALIZE = 5, OP_EW = 6, OP_MAXPOOL = 7, OP_AVGPOOL = 8,
  OP_CA_MLP = 9, OP_TABLE_FILL = 10, OP_MEMSET = 11, OP_ATT_MLP = 12, OP_SE_MLP = 13, OP_SHUFFLE = 14,
  OP_PWDW = 15, OP_DWPW = 16, OP_MSRB = 17, OP_CBAM = 18, OP_BNECK = 19, OP_STEMTAIL = 20,
  OP_CCW_POOL = 21, OP_CCW_GATE = 22, OP_CCW_DW = 23, OP_CCW_SHUFFLE = 24, OP_CCW_ARG = 25,
  OP_STEM_BWD = 101, OP_PW_BWD = 102, OP_DW_BWD = 103, OP_KXK_BWD = 104, OP_BN_BWD = 105, OP_EW_BWD = 106,
  OP_MAXPOOL_BWD = 107, OP_AVGPOOL_BWD = 108, OP_GATE_REDUCE = 109, OP_CA_MLP_BWD = 110, OP_ATT_MLP_BWD = 111, OP_SE_MLP_BWD = 112,
  OP_SHUFFLE_BWD = 113, OP_CBAM_BWD = 114,
};

// One captured launch sequence (hipGraph) of a phase for one set of pointers.
struct GraphEntry {
  int phase, training, nrep, seen;
  int64_t rstr;
  void *ws, *io0, *io1;
  uint64_t phash, ghash;
  hipGraphExec_t exec;
  uint64_t last_use;
};

struct Plan {
  std::vector<lhn_buf> bufs;
  std::vector<lhn_op> fwd, bwd;
  std::vector<uint8_t> pw_dz_dead;     // per backward op: an NHWC PW_BWD whose dz no later op touches (pw_dz_dead_at)
  std::vector<uint8_t> fwd_fin;        // per forward op: a convolution + BatchNorm whose finalize the next op takes (fwd_fin_consumer_at)
  std::vector<uint8_t> pair[2];        // per forward / backward op: 1 = first, 2 = second op of a pair launch (pair_at)
  std::vector<GraphEntry> graphs;     // LHN_GRAPH=1: replayed instead of ~150-400 individual launches
  uint64_t tick = 0;
  int graph_misses = 0;
};

static inline char* at(void* ws, int64_t off) { return off < 0 ? nullptr : static_cast<char*>(ws) + off; }

static lhn_view mkview(const Plan* P, void* ws, int buf, int coff, int C, bool with_gate = true) {
  const lhn_buf& b = P->bufs[buf];
  lhn_view v;
  v.pend = nullptr;      // (reserved)
  v.data = reinterpret_cast<float*>(at(ws, b.data_off));
  v.table = reinterpret_cast<const float*>(at(ws, b.table_off));
  v.gate = with_gate ? reinterpret_cast<const float*>(at(ws, b.gate_off)) : nullptr;
  v.N = b.N; v.H = b.H; v.W = b.W;
  v.cstride = b.C; v.coff = coff; v.C = C;
  return v;
}
static lhn_gradview mkgrad(const Plan* P, void* ws, int buf, bool use_coef) {
  const lhn_buf& b = P->bufs[buf];
  lhn_gradview g;
  g.dz = reinterpret_cast<const float*>(at(ws, b.grad_off));
  g.dpool = reinterpret_cast<const float*>(at(ws, b.dpool_off));
  g.coef = use_coef ? reinterpret_cast<const float*>(at(ws, b.coef_off)) : nullptr;
  return g;
}
template <typename T>
static inline T* prm(void* const* arr, int idx) { return idx < 0 ? nullptr : static_cast<T*>(arr[idx]); }
// BatchNorm slices of a gated buffer (lhn_bn_slices): packed (first channel << 16 | channels) in pk[0..1] (0 = none), byte offsets
// of the saved statistics in sv[0..1] and of the backward sums in sm[0..1] (NULL: sv only)
static lhn_bn_slices mkslices(void* ws, const int32_t* pk, const int64_t* sv, const int64_t* sm) {
  lhn_bn_slices s;
  memset(&s, 0, sizeof(s));
  for (int k = 0; k < 2; ++k)
    if (pk[k] > 0 && sv[k] >= 0) {
      const int j = s.n++;
      s.lo[j] = pk[k] >> 16;
      s.C[j] = pk[k] & 0xffff;
      s.save[j] = reinterpret_cast<const float*>(at(ws, sv[k]));
      s.sums[j] = (sm && sm[k] >= 0) ? reinterpret_cast<double*>(at(ws, sm[k])) : nullptr;
    }
  return s;
}

// conv op with a trailing BatchNorm: p[2..6] = gamma, beta, running_mean, running_var, num_batches_tracked,
// ws[1] = save(mean,invstd), ws[2] = arrival counter, f[0..2] = eps, momentum, slope
static bool conv_has_bn(const lhn_op& o) { return o.p[2] >= 0 || o.p[3] >= 0 || o.ws[1] >= 0; }
static lhn_bnfin mkfin(const Plan* P, void* ws, const lhn_op& o, void* const* params) {
  const lhn_buf& b = P->bufs[o.out_buf];
  lhn_bnfin f;
  f.counter = reinterpret_cast<uint32_t*>(at(ws, o.ws[2]));
  f.gamma = prm<const float>(params, o.p[2]);
  f.beta = prm<const float>(params, o.p[3]);
  f.running_mean = prm<float>(params, o.p[4]);
  f.running_var = prm<float>(params, o.p[5]);
  f.num_batches_tracked = prm<int64_t>(params, o.p[6]);
  f.table = reinterpret_cast<float*>(at(ws, b.table_off));
  f.save_mean_invstd = reinterpret_cast<float*>(at(ws, o.ws[1]));
  f.count = (double)b.N * b.H * b.W;
  f.cstride = b.C; f.coff = o.out_coff; f.C = o.out_C;
  f.eps = o.f[0]; f.momentum = o.f[1]; f.slope = o.f[2];
  f.conv_bias = prm<const float>(params, o.p[1]);   // biased conv + BN: the bias lives in the finalize only
  return f;
}
// LHN_FUSE_FINALIZE=1 (default 0): the last workgroup of a convolution folds the statistics and writes the table (lhn_bnfin) instead
// of a separate 1-workgroup launch.  Round 1 measured it SLOWER (one returning ticket atomic per workgroup on one word, ~88 tickets
// per us: 13.5 vs 12.9 ms per step of variant B); round 3 takes the tickets in two levels (32 group words + 1 top word) and folds
// the replicas with the whole block (lhn_last_block / lhn_bn_finalize_block_par).  Same box, alternating: variant B forward 2.550 ->
// 2.542 ms (97 instead of 149 launches), step 8.05 -> 8.06; Lite-HRNet step 35.85 -> 36.61; A 19.30 -> 19.42.  A finalize is its
// latency chain either way, so the separate launch stays the default.  Whole-plan runs only (SyncBatchNorm splits the op).
static bool fuse_finalize() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("LHN_FUSE_FINALIZE");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}
// LHN_BWD_FIN_CONSUMER (default 1, read once; 0 = the separate launches, for A/B runs): a BN_BWD op that stands directly in front of
// the backward of the convolution that owns the BatchNorm does not launch k_bn_bwd_finalize; the finished sums go to that
// convolution's entry point (lhn_bnbwdsrc: lhn_conv_dw_bwd4 / lhn_conv_pw_bwd4), whose kernel folds them in its prologue -- the
// coefficients have no other reader.  Unlike the producer-side fusion above this takes a launch AND its boundary out of the
// dependent chain, without tickets: the kernel boundary in front of the convolution orders the sums' atomics.  Whole-plan runs
// only, no padded channels; the op lists do not change.  Variant B: 50 of 52 pairs.
static bool bwd_fin_consumer() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("LHN_BWD_FIN_CONSUMER");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v == 1;
}
// LHN_FWD_FIN_CONSUMER (default 1, read once; 0 = the separate launches, for A/B runs): the same on the forward side.  A convolution +
// BatchNorm whose next op is a single-source NHWC depthwise or 1x1 convolution over exactly the BatchNorm's output view does not
// launch k_bn_finalize; the finished statistics go to that convolution's entry point (lhn_bnfinsrc: lhn_conv_dw_fwd4 /
// lhn_conv_pw_fwd3), whose kernel folds them in its prologue, under its first tile's loads, and leaves the table, mean | invstd and the
// running statistics in memory for every later reader.  Only where the route functions name a kernel with the fold: a consumer that
// would issue the launch itself gains nothing.  Decided once per plan (lhn_plan_fwd_fin_consumer); training whole-plan runs only
// (SyncBatchNorm ranges split the op at its second half and keep the launch), not with LHN_FUSE_FINALIZE, no padded channels, no unit
// the reference evaluates twice; the op lists do not change.  Variant B: 30 of 52 BatchNorms.
static bool fwd_fin_consumer() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("LHN_FWD_FIN_CONSUMER");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v == 1;
}
static bool fwd_fin_consumer_at(const Plan* P, const std::vector<lhn_op>& ops, size_t oi) {
  if (!fwd_fin_consumer() || fuse_finalize() || oi + 1 >= ops.size()) return false;
  const lhn_op &o = ops[oi], &nx = ops[oi + 1];
  const bool conv = o.kind == OP_STEM || o.kind == OP_PW || o.kind == OP_DW || (o.kind == OP_KXK && o.i[1] != 1);
  if (!conv || !conv_has_bn(o) || o.ws[0] < 0 || o.out_buf < 0 || (o.kind == OP_PW && (o.i[1] || o.i[2] > 0))) return false;
  if ((o.kind == OP_PW || o.kind == OP_DW) && (int)o.f[3] > 1) return false;
  if ((nx.kind != OP_DW && nx.kind != OP_PW) || nx.i[6] > 1) return false;
  if (nx.in_buf[0] != o.out_buf || nx.in_coff[0] != o.out_coff || nx.in_C[0] != o.out_C) return false;
  const lhn_buf& b = P->bufs[o.out_buf];
  if (b.table_off < 0) return false;
  const char* name;
  if (nx.kind == OP_DW)
    name = lhn_conv_dw_route(0, b.H, b.W, nx.in_C[0], nx.i[0], nx.i[1], nx.i[2], nx.i[3], LHN_DW_F_FINSRC | (nx.p[0] < 0 ? LHN_DW_F_NO_WEIGHT : 0), -1);
  else
    name = nx.i[1] ? nullptr
                   : lhn_conv_pw_route(0, b.N, b.H, b.W, nx.in_C[0], nx.out_C, nx.i[0], nx.i[2], nx.i[3],
                                       LHN_PW_F_FINSRC | (nx.ws[0] >= 0 ? LHN_PW_F_STATS : 0), -1);
  return name && strncmp(name, "lhn_bn_finalize", 15) != 0;
}
// Gate-gradient sums in the head's backward (lhn_gatesum, LHN_HEAD_STREAM, default on; not in deterministic mode): when the backward
// of an NCHW 1x1 (stride 1) STORES the gradient of its whole input buffer and the next op is the GATE_REDUCE of that buffer with
// T0 | T1, the 1x1 is the buffer's only reader -- any other reader's backward would stand between the two and accumulate -- and its
// dx is the buffer's complete dz.  lhn_conv_pw_bwd5 then adds dgate | T0 | T1 (in the head kernel's launch where it serves the shape,
// else by the same lhn_gate_bwd_reduce3 launch) and the GATE_REDUCE op is not launched.  CA_MLP_BWD reads the same arena.  Like the
// consumer-side finalize above this is decided here and not in the plan compiler: the op lists do not change.  Whole-plan runs only.
// Variant B: the pass over neck[1]'s buffer, 8 -> 7 k_gate_bwd_reduce launches per step.
static bool head_gate_fold_at(const Plan* P, const std::vector<lhn_op>& ops, size_t oi) {
  if (!lhn_head_stream_on() || lhn_deterministic_mode() || oi + 1 >= ops.size()) return false;
  const lhn_op &o = ops[oi], &nx = ops[oi + 1];
  if (o.kind != OP_PW_BWD || !o.i[1] || o.i[0] != 1 || o.i[2] != 1 || o.in_buf[0] < 0) return false;
  // the shapes k_head_bwd serves (no w_cols / w_rows given: the whole weight): every other head keeps its GATE_REDUCE op
  if (o.i[3] || o.i[4] || !lhn_head_shape(o.in_C[0], o.out_C, o.in_C[0], o.out_C)) return false;
  const lhn_buf& b = P->bufs[o.in_buf[0]];
  return o.in_coff[0] == 0 && o.in_C[0] == b.C && b.gate_off >= 0 && nx.kind == OP_GATE_REDUCE && nx.out_buf == o.in_buf[0] &&
         nx.out_coff == 0 && nx.out_C == b.C && nx.ws[3] >= 0 && nx.ws[4] >= 0;
}
// No dy store from the wide 1x1 backward (LHN_PW_BWD_DZ_DEAD of lhn_conv_pw_bwd6; LHN_PW_BWD_DY_STORE=1, read once, keeps the store
// for A/B runs).  dy = d loss / d (convolution output, in front of its BatchNorm) has two consumers, dX and dW of that convolution,
// both inside the PW_BWD launch; every other backward op reads a gradient buffer as d (the buffer's values as its readers see
// them), which is dz.  The backward list walks the forward records in reverse, so all writers of a view's gradient (its readers'
// backward ops) and the BN_BWD / GATE_REDUCE ops over it stand in FRONT of its producer's PW_BWD.  What can stand behind it and
// touch the same memory is another view of a shared gradient buffer (_alias_gradients: the hourglass Residual's conv3 and skip 1x1
// both take d(sum) from one buffer) -- and that op wants dz, which an in-place dy only equals because neither convolution has a
// BatchNorm.  So the flag would be right everywhere; it is still given only where the op list shows that nothing behind the PW_BWD
// touches the view's gradient at all (as a buffer's gradient, channels overlapping, or through a byte offset in ws[]): then the
// stored tensor has provably no reader and the bytes nobody looks at are the only difference.  Decided here, once per plan, and
// not in the plan compiler: the op lists do not change.  Whole-plan runs only.  Variant B: all 3 wide PW_BWD ops (2 MSRB closing
// 1x1 + the stem's 64 -> 128); A 8 of 8, M 6 of 6, H 4 of 5 (the Residual pair above keeps its store).
static bool pw_bwd_dy_store() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("LHN_PW_BWD_DY_STORE");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}
static bool pw_dz_dead_at(const Plan* P, const std::vector<lhn_op>& ops, size_t oi) {
  const lhn_op& o = ops[oi];
  if (o.kind != OP_PW_BWD || o.i[1] || o.out_buf < 0 || P->bufs[o.out_buf].grad_off < 0) return false;
  auto grad_bytes = [&](int buf, int64_t* lo, int64_t* hi) {
    const lhn_buf& b = P->bufs[buf];
    *lo = b.grad_off;
    *hi = b.grad_off + (int64_t)sizeof(float) * b.N * b.H * b.W * b.C;
    return b.grad_off >= 0;
  };
  int64_t lo, hi;
  grad_bytes(o.out_buf, &lo, &hi);
  const int oC = P->bufs[o.out_buf].C;
  auto touches = [&](int buf, int coff, int C) {
    int64_t a, b;
    if (buf < 0 || !grad_bytes(buf, &a, &b) || a >= hi || lo >= b) return false;
    // the same pixel stride: channel ranges decide; another layout over the same bytes: any overlap counts
    return a != lo || P->bufs[buf].C != oC || (coff < o.out_coff + o.out_C && o.out_coff < coff + C);
  };
  for (size_t k = oi + 1; k < ops.size(); ++k) {
    const lhn_op& q = ops[k];
    if (q.kind == OP_MEMSET) {
      if (q.ws[0] < hi && lo < q.ws[0] + q.ws[1]) return false;
      continue;
    }
    if (touches(q.out_buf, q.out_coff, q.out_C)) return false;
    for (int s = 0; s < 3; ++s)
      if (touches(q.in_buf[s], q.in_coff[s], q.in_C[s])) return false;
    for (int s = 0; s < 12; ++s)
      if (q.ws[s] >= lo && q.ws[s] < hi) return false;
  }
  return true;
}

// Pair launches (LHN_PAIR_LAUNCH, default 1, read once; 0 = single launches, for A/B runs).  An ungated RepBasicUnit returns a two-part
// tensor (left | depthwise(right), no copy), so every pool and combine over it stands in the op lists twice, once per half: adjacent,
// equal in geometry, independent.  Such a pair runs as ONE launch of the family's *_pair entry (blockIdx.y = the job, each job with
// the grid, replicas and arithmetic of its single launch: the same bits), the second op launches nothing.  The same for two
// consecutive convolution + BatchNorm ops that both keep their separate finalize launch (the two depthwise branches of an MSRB round):
// the first finalize has no reader before the second, waits, and runs as job 0 of lhn_bn_finalize_pair.  Decided here, once per plan,
// for whole-plan runs (lhn_plan_pair); the op lists do not change.  Variant B: 15 pool / combine pairs + 4 finalize pairs, 228 -> 209
// launches per step.
static bool pair_launch() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("LHN_PAIR_LAUNCH");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v == 1;
}
// what an op reads or writes: `pix` pixels of channels [coff, coff + C) at pixel stride cs, from byte offset `base` of the workspace
struct Region {
  int64_t base, pix;
  int cs, coff, C;
};
// the rule of pw_dz_dead_at: one base and pixel stride -> the channel ranges decide; another layout over the same bytes -> any overlap
static bool regions_meet(const Region& a, const Region& b) {
  if (a.base < 0 || b.base < 0) return false;
  if (a.base == b.base && a.cs == b.cs) return a.coff < b.coff + b.C && b.coff < a.coff + a.C;
  const int64_t alo = a.base + 4 * (int64_t)a.coff, ahi = a.base + 4 * ((a.pix - 1) * a.cs + a.coff + a.C);
  const int64_t blo = b.base + 4 * (int64_t)b.coff, bhi = b.base + 4 * ((b.pix - 1) * b.cs + b.coff + b.C);
  return alo < bhi && blo < ahi;
}
struct Access {
  std::vector<Region> rd, wr;
};
// reads and writes of a pool / combine op as data or as gradient (tables, gates and pooled gradients have no writer among these ops;
// BatchNorm-backward sums are only added to, atomically)
static bool pair_access(const Plan* P, const lhn_op& o, Access* A) {
  auto data = [&](int buf, int coff, int C) {
    const lhn_buf& b = P->bufs[buf];
    return Region{b.data_off, (int64_t)b.N * b.H * b.W, b.C, coff, C};
  };
  auto grad = [&](int buf, int coff, int C) {
    const lhn_buf& b = P->bufs[buf];
    return Region{b.grad_off, (int64_t)b.N * b.H * b.W, b.C, coff, C};
  };
  if (o.out_buf < 0 && o.kind != OP_AVGPOOL) return false;
  switch (o.kind) {
    case OP_MAXPOOL:
      if (o.in_buf[0] < 0) return false;
      A->rd.push_back(data(o.in_buf[0], o.in_coff[0], o.in_C[0]));
      A->wr.push_back(data(o.out_buf, o.out_coff, o.out_C));
      return true;
    case OP_EW:
      if (o.i[0] < 1 || o.i[0] > 3 || o.i[2] != 0) return false;                                   // product / bilinear: single
      for (int k = 0; k < o.i[0]; ++k) {
        if (o.in_buf[k] < 0) return false;
        A->rd.push_back(data(o.in_buf[k], o.in_coff[k], o.in_C[k]));
      }
      A->wr.push_back(data(o.out_buf, o.out_coff, o.out_C));
      return true;
    case OP_AVGPOOL: {
      if (o.in_buf[0] < 0 || o.ws[0] < 0 || o.ws[1] >= 0 || o.in_buf[1] >= 0) return false;          // STAT / COPY: single
      const lhn_buf& b = P->bufs[o.in_buf[0]];
      const int OH = o.i[0], OW = o.i[1];
      if (OH < 1 || OW < 1 || ((b.H + OH - 1) / OH + 1) * ((b.W + OW - 1) / OW + 1) <= 25) return false;      // the small-bin kernel: single
      A->rd.push_back(data(o.in_buf[0], o.in_coff[0], o.in_C[0]));
      A->wr.push_back(Region{o.ws[0], (int64_t)b.N * OH * OW, o.i[3] > 0 ? o.i[3] : o.in_C[0], o.i[4], o.in_C[0]});
      return true;
    }
    case OP_MAXPOOL_BWD: {
      if (o.in_buf[0] < 0) return false;
      const lhn_buf& xb = P->bufs[o.in_buf[0]];
      A->rd.push_back(data(o.in_buf[0], o.in_coff[0], o.in_C[0]));
      A->rd.push_back(grad(o.out_buf, o.out_coff, o.out_C));
      if (o.ws[2] >= 0) A->rd.push_back(Region{o.ws[2], (int64_t)xb.N * xb.H * xb.W, o.i[1], o.i[2], o.in_C[0]});
      if (o.ws[3] >= 0) A->rd.push_back(Region{o.ws[3], (int64_t)xb.N * (o.i[7] >> 16) * (o.i[7] & 0xffff), o.i[3], o.i[6], o.in_C[0]});
      A->wr.push_back(grad(o.in_buf[0], o.in_coff[0], o.in_C[0]));
      return true;
    }
    case OP_EW_BWD: {
      if ((o.i[1] != 0 && o.i[1] != 3) || o.f[0] == LHN_SLOPE_SILU || o.f[0] == LHN_SLOPE_RELU_SIGMOID) return false;
      A->rd.push_back(data(o.out_buf, o.out_coff, o.out_C));
      A->rd.push_back(grad(o.out_buf, o.out_coff, o.out_C));
      for (int k = 0; k < (o.i[1] == 3 ? 3 : 1) && o.in_buf[k] >= 0; ++k) {
        A->rd.push_back(data(o.in_buf[k], o.in_coff[k], o.in_C[k]));
        A->wr.push_back(grad(o.in_buf[k], o.in_coff[k], o.in_C[k]));
      }
      return !A->wr.empty();
    }
    default:
      return false;
  }
}
static bool same_shape(const Plan* P, int a, int b) {
  if ((a < 0) != (b < 0)) return false;
  if (a < 0) return true;
  const lhn_buf &x = P->bufs[a], &y = P->bufs[b];
  return x.N == y.N && x.H == y.H && x.W == y.W;
}
static bool conv_keeps_finalize_launch(const Plan* P, const std::vector<lhn_op>& ops, size_t oi) {
  const lhn_op& o = ops[oi];
  const bool conv = o.kind == OP_STEM || o.kind == OP_PW || o.kind == OP_DW || (o.kind == OP_KXK && o.i[1] != 1);
  if (!conv || !conv_has_bn(o) || o.ws[0] < 0 || o.out_buf < 0 || P->bufs[o.out_buf].table_off < 0) return false;
  if (o.kind == OP_PW && (o.i[1] || o.i[2] > 0)) return false;                                  // NCHW head, padded channel count
  if ((o.kind == OP_PW || o.kind == OP_DW) && (int)o.f[3] > 1) return false;                    // a unit the reference evaluates twice
  return !fuse_finalize() && !P->fwd_fin[oi];
}
// 0: ops oi and oi + 1 launch on their own; 1: a pool / combine pair; 2: a finalize pair (forward list only)
static int pair_at(const Plan* P, const std::vector<lhn_op>& ops, size_t oi, bool forward) {
  if (!pair_launch() || oi + 1 >= ops.size()) return 0;
  const lhn_op &a = ops[oi], &b = ops[oi + 1];
  if (forward && conv_keeps_finalize_launch(P, ops, oi) && conv_keeps_finalize_launch(P, ops, oi + 1)) {
    for (int k = 0; k < 3; ++k)      // the second convolution reads nothing of the first one's output view (its table is not there yet)
      if (b.in_buf[k] == a.out_buf && b.in_coff[k] < a.out_coff + a.out_C && a.out_coff < b.in_coff[k] + b.in_C[k]) return 0;
    if (b.kind == OP_STEM) return 0;
    // two separate BatchNorms: table slices, parameters, saved statistics
    if (a.out_buf == b.out_buf && a.out_coff < b.out_coff + b.out_C && b.out_coff < a.out_coff + a.out_C) return 0;
    for (int k = 2; k <= 6; ++k)
      if (a.p[k] >= 0 && a.p[k] == b.p[k]) return 0;
    if (a.ws[0] == b.ws[0] || (a.ws[1] >= 0 && a.ws[1] == b.ws[1])) return 0;
    return 2;
  }
  if (a.kind != b.kind) return 0;
  // the same mode bits and geometry
  if (a.kind == OP_EW && (a.i[0] != b.i[0] || a.i[2] != b.i[2])) return 0;
  if (a.kind == OP_EW_BWD && a.i[1] != b.i[1]) return 0;
  if (a.kind == OP_AVGPOOL && (a.i[0] != b.i[0] || a.i[1] != b.i[1])) return 0;
  if (a.out_C != b.out_C || !same_shape(P, a.out_buf, b.out_buf)) return 0;
  for (int k = 0; k < 3; ++k)
    if (!same_shape(P, a.in_buf[k], b.in_buf[k]) || (a.in_buf[k] >= 0 && a.in_C[k] != b.in_C[k])) return 0;
  Access A, B;
  if (!pair_access(P, a, &A) || !pair_access(P, b, &B)) return 0;
  for (const Region& w : A.wr) {
    for (const Region& q : B.wr)
      if (regions_meet(w, q)) return 0;
    for (const Region& q : B.rd)
      if (regions_meet(w, q)) return 0;
  }
  for (const Region& w : B.wr)
    for (const Region& q : A.rd)
      if (regions_meet(w, q)) return 0;
  return 1;
}

// arguments of one pool / combine op as its entry point takes them (single or as one job of a pair)
struct MaxpoolArgs {
  lhn_view x, y;
  lhn_bnsum bs;
  lhn_grad_adds ad;
  lhn_maxpool_job job;
};
static void mk_maxpool(const Plan* P, void* ws, const lhn_op& o, bool backward, MaxpoolArgs* A) {
  A->x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
  A->y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
  memset(&A->job, 0, sizeof(A->job));
  A->job.x = &A->x;
  A->job.y = &A->y;
  if (!backward) return;
  A->bs = mkbns(ws, o.ws[0], o.ws[1], o.i[4], o.i[5]);
  // ws[2] / i[1], i[2]: gradient of a plain sum that also reads x (base, pixel stride, first channel); ws[3] / i[3], i[6], i[7]:
  // gradient of an adaptive average pool of x (base, pixel stride, first channel, OH << 16 | OW) -- lhn_grad_adds
  lhn_grad_adds& ad = A->ad;
  memset(&ad, 0, sizeof(ad));
  if (o.ws[2] >= 0) {
    ad.same = reinterpret_cast<const float*>(at(ws, o.ws[2]));
    ad.same_cstride = o.i[1]; ad.same_coff = o.i[2];
  }
  if (o.ws[3] >= 0) {
    ad.pooled = reinterpret_cast<const float*>(at(ws, o.ws[3]));
    ad.pooled_cstride = o.i[3]; ad.pooled_coff = o.i[6];
    ad.OH = o.i[7] >> 16; ad.OW = o.i[7] & 0xffff;
  }
  A->job.dy = reinterpret_cast<const float*>(at(ws, P->bufs[o.out_buf].grad_off));
  A->job.dx = reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off));
  A->job.dx_accumulate = o.i[0];
  A->job.bns = A->bs.sums ? &A->bs : nullptr;
  A->job.adds = (ad.same || ad.pooled) ? &ad : nullptr;
}
struct EwArgs {
  lhn_view srcs[3], d;
  float coef[3];
  float* dsrcs[3];
  int acc[3];
  lhn_bnsum bsv[3];
  const lhn_bnsum* bsp[3];
  lhn_ew_job job;
};
static void mk_ew_fwd(const Plan* P, void* ws, const lhn_op& o, EwArgs* A) {
  for (int k = 0; k < o.i[0]; ++k) A->srcs[k] = mkview(P, ws, o.in_buf[k], o.in_coff[k], o.in_C[k]);
  A->d = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
  for (int k = 0; k < 3; ++k) A->coef[k] = o.f[4 + k];
  memset(&A->job, 0, sizeof(A->job));
  A->job.srcs = A->srcs;
  A->job.nsrc = o.i[0];
  A->job.coef = o.i[1] ? A->coef : nullptr;      // i[1]: coefficients given; i[2]: mode
  A->job.dst = &A->d;
  A->job.out_slope = o.f[0];
  A->job.mode = o.i[2];
}
// the sum forms of EW_BWD.  i[1] == 0: one source, accumulate flag i[0], its producer's sums ws[0..1] / i[4..5].  i[1] == 3: 2 or 3 sources
// of the destination's resolution in one pass: in_buf[0..2]; accumulate flags i[0], i[2], i[3]; their producers' sums ws[0..5],
// (C, coff) in i[4..7] and f[4..5]
static void mk_ew_bwd(const Plan* P, void* ws, const lhn_op& o, EwArgs* A) {
  const lhn_buf& db = P->bufs[o.out_buf];
  A->d = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
  const bool multi = o.i[1] == 3;
  A->acc[0] = o.i[0]; A->acc[1] = o.i[2]; A->acc[2] = o.i[3];
  A->bsv[0] = mkbns(ws, o.ws[0], o.ws[1], o.i[4], o.i[5]);
  A->bsv[1] = multi ? mkbns(ws, o.ws[2], o.ws[3], o.i[6], o.i[7]) : mkbns(ws, -1, -1, 0, 0);
  A->bsv[2] = multi ? mkbns(ws, o.ws[4], o.ws[5], (int)o.f[4], (int)o.f[5]) : mkbns(ws, -1, -1, 0, 0);
  int ns = 0;
  for (; ns < (multi ? 3 : 1) && o.in_buf[ns] >= 0; ++ns) {
    A->srcs[ns] = mkview(P, ws, o.in_buf[ns], o.in_coff[ns], o.in_C[ns]);
    A->dsrcs[ns] = reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[ns]].grad_off));
    A->bsp[ns] = A->bsv[ns].sums ? &A->bsv[ns] : nullptr;
  }
  memset(&A->job, 0, sizeof(A->job));
  A->job.srcs = A->srcs;
  A->job.nsrc = ns;
  A->job.dst = &A->d;
  A->job.out_slope = o.f[0];
  A->job.ddst = reinterpret_cast<const float*>(at(ws, db.grad_off));
  A->job.dst_dpool = reinterpret_cast<const float*>(at(ws, db.dpool_off));
  A->job.dsrcs = A->dsrcs;
  A->job.accumulate = A->acc;
  A->job.bns = A->bsp;
}
struct AvgpoolArgs {
  lhn_view x;
  lhn_avgpool_job job;
};
static void mk_avgpool(const Plan* P, void* ws, const lhn_op& o, AvgpoolArgs* A) {      // the plain form (no statistics, no copy source)
  A->x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0], o.i[2] == 0);
  memset(&A->job, 0, sizeof(A->job));
  A->job.x = &A->x;
  A->job.out = reinterpret_cast<float*>(at(ws, o.ws[0]));
  A->job.OH = o.i[0]; A->job.OW = o.i[1];
  A->job.out_cstride = o.i[3] > 0 ? o.i[3] : A->x.C;
  A->job.out_coff = o.i[4];
}

// creal: channels the BatchNorm really has when the convolution's output view is padded to a multiple of 4 (f.C then is the
// layout of the statistics); repeat: the reference evaluates some units twice per forward (lite_hrnet.py:192-197), which
// moves their running statistics twice -- the table is the same both times.
static int sep_finalize(const lhn_bnfin& f, const double* stats, int training, void* stream, int creal = 0, int repeat = 1) {
  int rc = 0;
  for (int r = 0; r < (training ? (repeat < 1 ? 1 : repeat) : 1) && !rc; ++r)
    rc = lhn_bn_finalize2(training ? stats : nullptr, f.gamma, f.beta, f.running_mean, f.running_var,
                          training ? f.num_batches_tracked : nullptr, f.table, f.cstride, f.coff, creal > 0 ? creal : f.C, f.C,
                          training ? f.save_mean_invstd : nullptr, f.count, f.eps, f.momentum, f.slope, training, f.conv_bias, stream);
  return rc;
}

extern "C" {

void* lhn_plan_create(const lhn_buf* bufs, int nbufs, const lhn_op* fwd, int nfwd, const lhn_op* bwd, int nbwd) {
  if (!bufs || nbufs <= 0 || !fwd || nfwd <= 0) {
    lhn_set_error("lhn_plan_create: empty plan");
    return nullptr;
  }
  Plan* p = new Plan();
  p->bufs.assign(bufs, bufs + nbufs);
  p->fwd.assign(fwd, fwd + nfwd);
  if (bwd && nbwd > 0) p->bwd.assign(bwd, bwd + nbwd);
  for (const auto* lst : {&p->fwd, &p->bwd})
    for (const lhn_op& o : *lst) {
      bool ok = o.out_buf < nbufs;
      for (int k = 0; k < 3; ++k) ok = ok && o.in_buf[k] < nbufs;
      if (!ok) {
        lhn_set_error("lhn_plan_create: op kind %d references buffer out of range", o.kind);
        delete p;
        return nullptr;
      }
    }
  p->fwd_fin.resize(p->fwd.size());
  for (size_t oi = 0; oi < p->fwd.size(); ++oi) p->fwd_fin[oi] = fwd_fin_consumer_at(p, p->fwd, oi) ? 1 : 0;
  p->pw_dz_dead.resize(p->bwd.size());
  for (size_t oi = 0; oi < p->bwd.size(); ++oi) p->pw_dz_dead[oi] = pw_dz_dead_at(p, p->bwd, oi) ? 1 : 0;
  for (int phase = 0; phase < 2; ++phase) {      // left to right: an op belongs to one pair at most
    const std::vector<lhn_op>& ops = phase == 0 ? p->fwd : p->bwd;
    std::vector<uint8_t>& pr = p->pair[phase];
    pr.assign(ops.size(), 0);
    for (size_t oi = 0; oi + 1 < ops.size(); ++oi)
      if (!pr[oi] && pair_at(p, ops, oi, phase == 0)) {
        pr[oi] = 1;
        pr[oi + 1] = 2;
      }
  }
  return p;
}

int lhn_plan_pair(void* plan, int phase, int index) {
  const Plan* p = static_cast<const Plan*>(plan);
  if (!p || phase < 0 || phase > 1 || index < 0 || (size_t)index >= p->pair[phase].size()) return -1;
  return p->pair[phase][index];
}

int lhn_plan_head_gate_fold(void* plan) {
  const Plan* p = static_cast<const Plan*>(plan);
  if (!p) return -1;
  for (size_t oi = 0; oi + 1 < p->bwd.size(); ++oi)
    if (head_gate_fold_at(p, p->bwd, oi)) return (int)oi + 1;
  return -1;
}

int lhn_plan_pw_dz_dead(void* plan, int bwd_index) {
  const Plan* p = static_cast<const Plan*>(plan);
  if (!p || bwd_index < 0 || (size_t)bwd_index >= p->pw_dz_dead.size()) return -1;
  return p->pw_dz_dead[bwd_index];
}

int lhn_plan_fwd_fin_consumer(void* plan, int fwd_index) {
  const Plan* p = static_cast<const Plan*>(plan);
  if (!p || fwd_index < 0 || (size_t)fwd_index >= p->fwd_fin.size()) return -1;
  return p->fwd_fin[fwd_index];
}

void lhn_plan_destroy(void* plan) {
  Plan* p = static_cast<Plan*>(plan);
  if (!p) return;
  for (GraphEntry& g : p->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  delete p;
}

// Ops are numbered in HALF-steps: step 2*i = the op's main launches, step 2*i+1 = its statistics consumer (BatchNorm
// finalize, second half of an attention op).  SyncBatchNorm runs [.., 2*i] / all-reduce / [2*i+1, ..]; a plain run is
// the whole range.  count_scale = world size (statistics are over N*world samples), pgrad_scale = 1/world for the
// d(gamma), d(beta) that come out of globally reduced sums.
static int run_ops(const Plan* P, int phase, void* ws, void* const* params, void* const* grads, void* const* io, int mode,
                   int nrep, int64_t rstr, void* stream, size_t sb = 0, size_t se = (size_t)-1, double cscale = 1.0,
                   float pscale = 1.f) {
  // mode bit 0 = training (batch statistics); bit 1 (eval only, LHN_RUN_TABLES_CURRENT) = the per-buffer (scale, shift,
  // slope) tables already hold the running-statistics BatchNorms / deployed biases of the current parameters: skip the
  // launches that only rebuild them (52 of variant B's ~200 forward launches)
  const int training = mode & 1;
  const bool skip_tables = (mode & 2) != 0 && !training;
  const std::vector<lhn_op>& ops = phase == 0 ? P->fwd : P->bwd;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = 0;
  const bool whole = (sb == 0 && se >= 2 * ops.size());
  lhn_bnbwdsrc cfin;                    // finalize source of the BN_BWD op in front of op cfin_for (consumer-side finalize)
  size_t cfin_for = (size_t)-1;
  lhn_bnfinsrc ffin;                    // finalize source of the forward convolution in front of op ffin_for (fwd_fin_consumer_at)
  size_t ffin_for = (size_t)-1;
  // the BatchNorm of forward op oi is finalized by op oi + 1: no launch here, the statistics travel with `fin`
  auto hand_over = [&](size_t oi, const lhn_bnfin& fin, const double* stats) {
    if (phase != 0 || !training || !whole || skip_tables || !P->fwd_fin[oi]) return false;
    ffin.stats = stats;
    ffin.gamma = fin.gamma; ffin.beta = fin.beta; ffin.conv_bias = fin.conv_bias;
    ffin.running_mean = fin.running_mean; ffin.running_var = fin.running_var; ffin.num_batches_tracked = fin.num_batches_tracked;
    ffin.table = fin.table; ffin.save_mean_invstd = fin.save_mean_invstd;
    ffin.count = fin.count;
    ffin.cstride = fin.cstride; ffin.coff = fin.coff; ffin.C = fin.C;
    ffin.eps = fin.eps; ffin.momentum = fin.momentum; ffin.slope = fin.slope;
    ffin_for = oi + 1;
    return true;
  };
  // pair launches (pair_at): whole-plan runs only.  pr[oi] == 1: op oi launches for itself and op oi + 1; 2: launches nothing
  const uint8_t* pr = whole ? P->pair[phase].data() : nullptr;
  lhn_bnfin dfin;                       // the finalize of the convolution in front of op dfin_for, waiting for that op's
  const double* dstats = nullptr;
  size_t dfin_for = (size_t)-1;
  auto finalize = [&](size_t oi, const lhn_bnfin& fin, const double* stats, int creal, int repeat) -> int {
    if (pr && pr[oi] == 1) {
      dfin = fin;
      dstats = stats;
      dfin_for = oi + 1;
      return 0;
    }
    if (pr && pr[oi] == 2 && dfin_for == oi) {
      lhn_bnfin fa = dfin, fb = fin;
      if (!training) {      // as sep_finalize: the table from the running statistics, nothing else is touched
        fa.num_batches_tracked = fb.num_batches_tracked = nullptr;
        fa.save_mean_invstd = fb.save_mean_invstd = nullptr;
      }
      return lhn_bn_finalize_pair(training ? dstats : nullptr, &fa, fa.C, training ? stats : nullptr, &fb, fb.C, training, stream);
    }
    return sep_finalize(fin, stats, training, stream, creal, repeat);
  };
  size_t gfold_at = (size_t)-1;         // the GATE_REDUCE op whose sums the head's backward in front of it added (head_gate_fold_at)
  for (size_t oi = 0; oi < ops.size() && rc == 0; ++oi) {
    const lhn_op& o = ops[oi];
    const bool deferred = false;      // (round 2's deferred finalize is gone)
    // fused finalize (last workgroup of the convolution): whole-plan runs only (SyncBatchNorm splits the op at the exchange), not
    // for padded channel counts (the in-kernel form has one channel count) nor for units the reference evaluates twice
    const bool is_conv = o.kind == OP_STEM || o.kind == OP_PW || o.kind == OP_DW || o.kind == OP_KXK;
    const bool fz = is_conv && training && fuse_finalize() && whole && !(o.kind == OP_PW && o.i[2] > 0) &&
                    !((o.kind == OP_PW || o.kind == OP_DW) && (int)o.f[3] > 1);
    const bool h0 = 2 * oi >= sb && 2 * oi < se, h1 = 2 * oi + 1 >= sb && 2 * oi + 1 < se;
    if (!h0 && !h1) continue;
    const bool two_half = o.kind == OP_STEM || o.kind == OP_PW || o.kind == OP_DW || o.kind == OP_KXK || o.kind == OP_CA_MLP ||
                          o.kind == OP_ATT_MLP || o.kind == OP_BN_BWD || o.kind == OP_CA_MLP_BWD || o.kind == OP_ATT_MLP_BWD;
    if (!two_half && !h0) continue;
    const int stage = (h0 && h1) ? 0 : (h0 ? 1 : 2);
    switch (o.kind) {
      case OP_MEMSET: {
        if (hipMemsetAsync(at(ws, o.ws[0]), 0, (size_t)o.ws[1], s) != hipSuccess) {
          lhn_set_error("lhn_plan_run: memset failed");
          rc = 2;
        }
        break;
      }
      case OP_TABLE_FILL: {
        if (skip_tables) break;
        const lhn_buf& b = P->bufs[o.out_buf];
        if (o.i[0])  // deployed conv: (1, bias, slope)
          rc = lhn_table_bias(reinterpret_cast<float*>(at(ws, b.table_off)), b.C, o.out_coff, o.out_C, prm<const float>(params, o.p[0]), o.f[2], stream);
        else
          rc = lhn_table_fill(reinterpret_cast<float*>(at(ws, b.table_off)), b.C, o.out_coff, o.out_C, o.f[0], o.f[1], o.f[2], stream);
        break;
      }
      case OP_STEM: {
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        const bool bn = conv_has_bn(o);
        lhn_bnfin fin;
        if (bn) {
          fin = mkfin(P, ws, o, params);
          fin.count *= cscale;
        }
        if (h0) rc = lhn_conv_stem_fwd(static_cast<const float*>(io[0]), prm<const float>(params, o.p[0]), &y,
                               (training && o.ws[0] >= 0) ? reinterpret_cast<double*>(at(ws, o.ws[0])) : nullptr, o.i[3], o.i[4], o.i[0], o.i[1],
                               o.i[2], (bn && fz) ? &fin : nullptr, stream);
        if (!rc && bn && h1 && !skip_tables && !deferred && !fz && !hand_over(oi, fin, reinterpret_cast<const double*>(at(ws, o.ws[0]))))
          rc = finalize(oi, fin, reinterpret_cast<const double*>(at(ws, o.ws[0])), 0, 1);
        break;
      }
      case OP_PW: {
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y;
        float* nchw = nullptr;
        if (o.i[1]) {  // NCHW head: geometry from the input, channels from out_C
          y = x;
          y.data = nullptr; y.table = nullptr; y.gate = nullptr; y.pend = nullptr;
          y.cstride = o.out_C; y.coff = 0; y.C = o.out_C;
          nchw = static_cast<float*>(io[1]);
        } else {
          y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        }
        const bool bn = !o.i[1] && conv_has_bn(o);
        lhn_bnfin fin;
        if (bn) {
          fin = mkfin(P, ws, o, params);
          fin.count *= cscale;
        }
        // i[2], i[3] = real rows / columns of the weight tensor when the views are padded to a multiple of 4 (0 = the views');
        // i[4], i[5] = stack index / number of stacks of an NCHW output [N, S, K, H, W] (hourglassnet.py:136)
        lhn_pw_opts po;
        memset(&po, 0, sizeof(po));
        po.w_rows = o.i[2]; po.w_cols = o.i[3];
        lhn_view extra[2];
        if (o.i[6] > 1) {      // i[6] sources summed on load: in_buf[1..], coefficients f[4..6]
          po.n_extra = o.i[6] - 1;
          for (int e = 0; e < po.n_extra; ++e) {
            extra[e] = mkview(P, ws, o.in_buf[e + 1], o.in_coff[e + 1], o.in_C[e + 1]);
          }
          po.extra = extra;
          for (int e = 0; e < 3; ++e) po.coef[e] = o.f[4 + e];
        }
        // ws[4] >= 0 (plans with a backward): the summed input is also written to the buffer at that byte offset, ws[5] = pixel
        // stride * 65536 + first channel (lhn_pw_opts.sum_out)
        lhn_view sumv;
        if (o.i[6] > 1 && o.ws[4] >= 0) {
          sumv = x;
          sumv.data = reinterpret_cast<float*>(at(ws, o.ws[4]));
          sumv.table = nullptr; sumv.gate = nullptr; sumv.pend = nullptr;
          sumv.cstride = (int)(o.ws[5] >> 16); sumv.coff = (int)(o.ws[5] & 0xffff);
          po.sum_out = &sumv;
        }
        if (nchw && o.i[5] > 1) {
          const int64_t khw = (int64_t)o.out_C * y.H * y.W;
          nchw += (int64_t)o.i[4] * khw;
          po.nchw_batch_stride = (int64_t)o.i[5] * khw;
        }
        if (h0) rc = lhn_conv_pw_fwd3(&x, prm<const float>(params, o.p[0]), bn ? nullptr : prm<const float>(params, o.p[1]), &y,
                              (training && o.ws[0] >= 0) ? reinterpret_cast<double*>(at(ws, o.ws[0])) : nullptr, o.i[0], nchw,
                              (bn && fz) ? &fin : nullptr, &po, ffin_for == oi ? &ffin : nullptr, stream);
        if (!rc && bn && h1 && !skip_tables && !deferred && !fz && !hand_over(oi, fin, reinterpret_cast<const double*>(at(ws, o.ws[0]))))
          rc = finalize(oi, fin, reinterpret_cast<const double*>(at(ws, o.ws[0])), o.i[2], (int)o.f[3]);
        break;
      }
      case OP_DW: {
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        const bool bn = conv_has_bn(o);
        lhn_bnfin fin;
        if (bn) {
          fin = mkfin(P, ws, o, params);
          fin.count *= cscale;
        }
        lhn_view extra;
        const float coef2[2] = {o.f[4], o.f[5]};
        if (o.i[6] > 1) {                                                                 // second source summed on load
          extra = mkview(P, ws, o.in_buf[1], o.in_coff[1], o.in_C[1]);
        }
        lhn_view sumv;           // ws[4], ws[5]: see OP_PW
        const bool so = o.i[6] > 1 && o.ws[4] >= 0;
        if (so) {
          sumv = x;
          sumv.data = reinterpret_cast<float*>(at(ws, o.ws[4]));
          sumv.table = nullptr; sumv.gate = nullptr; sumv.pend = nullptr;
          sumv.cstride = (int)(o.ws[5] >> 16); sumv.coff = (int)(o.ws[5] & 0xffff);
        }
        if (h0) rc = lhn_conv_dw_fwd4(&x, prm<const float>(params, o.p[0]), &y,
                              (training && o.ws[0] >= 0) ? reinterpret_cast<double*>(at(ws, o.ws[0])) : nullptr, o.i[0], o.i[1], o.i[2], o.i[3],
                              (bn && fz) ? &fin : nullptr, o.i[6] > 1 ? &extra : nullptr, coef2,
                              so ? &sumv : nullptr, ffin_for == oi ? &ffin : nullptr, stream);
        if (!rc && bn && h1 && !skip_tables && !deferred && !fz && !hand_over(oi, fin, reinterpret_cast<const double*>(at(ws, o.ws[0]))))
          rc = finalize(oi, fin, reinterpret_cast<const double*>(at(ws, o.ws[0])), 0, (int)o.f[3]);
        break;
      }
      case OP_KXK: {
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        const bool bn = conv_has_bn(o);
        lhn_bnfin fin;
        if (bn) {
          fin = mkfin(P, ws, o, params);
          fin.count *= cscale;
        }
        if (o.i[1] == 1) {  // bf16x3 (PlanBuilder.mark_bf16x3): the split-bf16 MFMA kernel; ws[3] holds the split weights.  Inference plans
          // only.  The scratch is a function of the parameters like the tables: LHN_RUN_TABLES_CURRENT keeps it too.
          if (training) {
            lhn_set_error("lhn_plan_run: a bf16x3 3x3 launch has no batch statistics (inference plans only)");
            rc = 1;
            break;
          }
          if (h0) rc = lhn_conv_kxk_fwd_bf16x3(&x, prm<const float>(params, o.p[0]), &y, o.ws[3] >= 0 ? at(ws, o.ws[3]) : nullptr,
                                               skip_tables ? 0 : 1, stream);
          if (!rc && bn && h1 && !skip_tables) rc = sep_finalize(fin, nullptr, 0, stream);
          break;
        }
        if (h0) rc = lhn_conv_kxk_fwd(&x, prm<const float>(params, o.p[0]), &y,
                              (training && o.ws[0] >= 0) ? reinterpret_cast<double*>(at(ws, o.ws[0])) : nullptr, o.i[0],
                              (bn && fz) ? &fin : nullptr,
                              o.ws[3] >= 0 ? reinterpret_cast<float*>(at(ws, o.ws[3])) : nullptr, stream);
        if (!rc && bn && h1 && !skip_tables && !deferred && !fz && !hand_over(oi, fin, reinterpret_cast<const double*>(at(ws, o.ws[0]))))
          rc = finalize(oi, fin, reinterpret_cast<const double*>(at(ws, o.ws[0])), 0, 1);
        break;
      }
      case OP_PWDW: {  // in: x, the intermediate buffer (only its table exists); p: w1, w2.  Inference plans only.
        if (training) {
          lhn_set_error("lhn_plan_run: a fused 1x1 -> depthwise launch has no batch statistics (inference plans only)");
          rc = 1;
          break;
        }
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        rc = lhn_conv_pw_dw3_fwd(&x, prm<const float>(params, o.p[0]), reinterpret_cast<const float*>(at(ws, P->bufs[o.in_buf[1]].table_off)),
                                 prm<const float>(params, o.p[1]), &y, stream);
        break;
      }
      case OP_DWPW: {  // in: x, the intermediate buffer (only its table exists); p: w_dw, w_pw, bias or -1; i[0] = dilation.  Inference plans only.
        if (training) {
          lhn_set_error("lhn_plan_run: a fused depthwise -> 1x1 launch has no batch statistics (inference plans only)");
          rc = 1;
          break;
        }
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        rc = lhn_conv_dw3_pw_fwd(&x, prm<const float>(params, o.p[0]), o.i[0], reinterpret_cast<const float*>(at(ws, P->bufs[o.in_buf[1]].table_off)),
                                 prm<const float>(params, o.p[1]), prm<const float>(params, o.p[2]), &y, stream);
        break;
      }
      case OP_BNECK: {  // BottleNeck in one launch.  in: x and the outputs of the first 1x1 and of the 3x3 (only their tables exist); ws[0]: table
        // of the second 1x1's output, ws[1]: tap-major scratch of the 3x3's weights; p: w1, b1 or -1, w2, w3, b3 or -1; f[0] = out_slope.
        // Inference plans only.  The scratch is a function of the parameters like the tables: LHN_RUN_TABLES_CURRENT keeps it too.
        if (training) {
          lhn_set_error("lhn_plan_run: a fused BottleNeck launch has no batch statistics (inference plans only)");
          rc = 1;
          break;
        }
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        rc = lhn_bottleneck_fwd_impl(&x, o.in_C[1], prm<const float>(params, o.p[0]), prm<const float>(params, o.p[1]),
                                     reinterpret_cast<const float*>(at(ws, P->bufs[o.in_buf[1]].table_off)), prm<const float>(params, o.p[2]),
                                     reinterpret_cast<const float*>(at(ws, P->bufs[o.in_buf[2]].table_off)), prm<const float>(params, o.p[3]),
                                     prm<const float>(params, o.p[4]), reinterpret_cast<const float*>(at(ws, o.ws[0])), o.f[0], &y,
                                     reinterpret_cast<float*>(at(ws, o.ws[1])), skip_tables ? 0 : 1, stream);
        break;
      }
      case OP_STEMTAIL: {  // the stem after its first convolution in one launch.  in[0]: x (i[0] = K > 0: the depthwise convolution's input;
        // K == 0: t itself), in[1]: t, in[2]: u (of both only the tables exist; K == 0: t's is x's own); ws[0]: table of the concatenation
        // buffer, whose first in_C[2] channels are v's, i[1]: its channel count; ws[1]: tap-major scratch of the 3x3's weights; p: w_dw, bT,
        // w1, b1, w2, b2, w3, b3 (-1 = none).  Inference plans only; the scratch follows LHN_RUN_TABLES_CURRENT like OP_BNECK's.
        if (training) {
          lhn_set_error("lhn_plan_run: a fused stem launch has no batch statistics (inference plans only)");
          rc = 1;
          break;
        }
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        rc = lhn_stem_tail_fwd_impl(&x, o.i[0], prm<const float>(params, o.p[0]), prm<const float>(params, o.p[1]),
                                    o.i[0] ? reinterpret_cast<const float*>(at(ws, P->bufs[o.in_buf[1]].table_off)) : nullptr,
                                    prm<const float>(params, o.p[2]), prm<const float>(params, o.p[3]),
                                    reinterpret_cast<const float*>(at(ws, P->bufs[o.in_buf[2]].table_off)), prm<const float>(params, o.p[4]),
                                    prm<const float>(params, o.p[5]), reinterpret_cast<const float*>(at(ws, o.ws[0])), o.i[1],
                                    prm<const float>(params, o.p[6]), prm<const float>(params, o.p[7]), &y,
                                    reinterpret_cast<float*>(at(ws, o.ws[1])), skip_tables ? 0 : 1, 0, stream);
        break;
      }
      case OP_MSRB: {  // one MSRB round.  in[0], in[1]: the x views of the two halves; in[2] and i[1..3] (buffer, first channel, channels):
        // their extra sources when i[6] > 1, coefficients f[4..5] as OP_DW; out: the whole y view; p: the two weights; ws[0], ws[1]:
        // pooled / scratch or -1; i[0] = OH.  Inference plans only.
        if (training) {
          lhn_set_error("lhn_plan_run: a fused MSRB round has no batch statistics (inference plans only)");
          rc = 1;
          break;
        }
        const lhn_view x[2] = {mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]), mkview(P, ws, o.in_buf[1], o.in_coff[1], o.in_C[1])};
        lhn_view extra[2];
        const bool two = o.i[6] > 1;
        if (two) {
          if (o.in_buf[2] < 0 || o.i[1] < 0 || o.i[1] >= (int)P->bufs.size()) {
            lhn_set_error("lhn_plan_run: fused MSRB round: extra source out of range");
            rc = 1;
            break;
          }
          extra[0] = mkview(P, ws, o.in_buf[2], o.in_coff[2], o.in_C[2]);
          extra[1] = mkview(P, ws, o.i[1], o.i[2], o.i[3]);
        }
        const float coef2[2] = {o.f[4], o.f[5]};
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C, false);      // (its gate is written by the attention MLP behind this launch)
        rc = lhn_msrb_round_fwd(x, two ? extra : nullptr, two ? coef2 : nullptr, prm<const float>(params, o.p[0]), prm<const float>(params, o.p[1]),
                                &y, reinterpret_cast<float*>(at(ws, o.ws[0])), o.i[0], o.i[0], at(ws, o.ws[1]), stream);
        break;
      }
      case OP_CCW_ARG:  // one branch of a ConditionalChannelWeighting block, read by the CCW launch behind it; launches nothing
        break;
      case OP_CCW_POOL:
      case OP_CCW_DW:
      case OP_CCW_SHUFFLE: {  // i[0] = B; the B ops in front are OP_CCW_ARG, one per branch: in[0] = x2, in[1] = x1, in[2] = y (raw depthwise
        // output), out = the shuffled output, p = w_dw, SpatialWeighting's w1, b1, w2, b2, i[0] = its J.  POOL: out = the pooled
        // concatenation (whole buffer); DW: in[0] = g (whole buffer), ws[0] = scratch; SHUFFLE: ws[0] = scratch.  Inference plans only.
        if (training) {
          lhn_set_error("lhn_plan_run: a grouped channel-weighting launch has no batch statistics (inference plans only)");
          rc = 1;
          break;
        }
        const int B = o.i[0];
        if (B < 2 || B > 4 || oi < (size_t)B) {
          lhn_set_error("lhn_plan_run: channel-weighting op at index %zu: %d branches", oi, B);
          rc = 1;
          break;
        }
        lhn_view x2[4], x1[4], y[4], out[4];
        const float* w[4];
        lhn_ccw_se se[4];
        for (int b = 0; b < B && rc == 0; ++b) {
          const lhn_op& g = ops[oi - B + b];
          if (g.kind != OP_CCW_ARG || g.in_buf[0] < 0 || g.in_buf[1] < 0 || g.in_buf[2] < 0 || g.out_buf < 0) {
            lhn_set_error("lhn_plan_run: channel-weighting op at index %zu: branch %d is not described", oi, b);
            rc = 1;
            break;
          }
          x2[b] = mkview(P, ws, g.in_buf[0], g.in_coff[0], g.in_C[0]);
          x1[b] = mkview(P, ws, g.in_buf[1], g.in_coff[1], g.in_C[1]);
          y[b] = mkview(P, ws, g.in_buf[2], g.in_coff[2], g.in_C[2], false);      // (its gate lives in the shuffle launch)
          out[b] = mkview(P, ws, g.out_buf, g.out_coff, g.out_C);
          w[b] = prm<const float>(params, g.p[0]);
          se[b].w1 = prm<const float>(params, g.p[1]); se[b].b1 = prm<const float>(params, g.p[2]);
          se[b].w2 = prm<const float>(params, g.p[3]); se[b].b2 = prm<const float>(params, g.p[4]);
          se[b].J = g.i[0];
        }
        if (rc) break;
        if ((o.kind == OP_CCW_POOL && o.out_buf < 0) || (o.kind == OP_CCW_DW && o.in_buf[0] < 0)) {
          lhn_set_error("lhn_plan_run: channel-weighting op at index %zu: missing buffer", oi);
          rc = 1;
          break;
        }
        if (o.kind == OP_CCW_POOL)
          rc = lhn_ccw_pool_fwd(x2, B, reinterpret_cast<float*>(at(ws, P->bufs[o.out_buf].data_off)), stream);
        else if (o.kind == OP_CCW_DW)
          rc = lhn_ccw_dw_fwd(x2, B, reinterpret_cast<const float*>(at(ws, P->bufs[o.in_buf[0]].data_off)), w, y, at(ws, o.ws[0]), stream);
        else
          rc = lhn_ccw_shuffle_fwd(x1, y, B, se, at(ws, o.ws[0]), out, stream);
        break;
      }
      case OP_CCW_GATE: {  // in[0] = pooled (whole buffer), in[1] / in[2] = the outputs of the two 1x1 convolutions (only their tables exist:
        // eval BatchNorm with the bias folded in), out = g (whole buffer); p = W1, W2; i[0] = mid.  Inference plans only.
        if (training) {
          lhn_set_error("lhn_plan_run: a grouped channel-weighting launch has no batch statistics (inference plans only)");
          rc = 1;
          break;
        }
        if (o.in_buf[0] < 0 || o.in_buf[1] < 0 || o.in_buf[2] < 0 || o.out_buf < 0) {
          lhn_set_error("lhn_plan_run: channel-weighting gate at index %zu: missing buffer", oi);
          rc = 1;
          break;
        }
        const lhn_buf &pb = P->bufs[o.in_buf[0]], &b1 = P->bufs[o.in_buf[1]], &b2 = P->bufs[o.in_buf[2]], &gb = P->bufs[o.out_buf];
        if (gb.C != pb.C || gb.H != pb.H || gb.W != pb.W) {
          lhn_set_error("lhn_plan_run: channel-weighting gate at index %zu: pooled and g differ", oi);
          rc = 1;
          break;
        }
        rc = lhn_ccw_gate_fwd(reinterpret_cast<const float*>(at(ws, pb.data_off)), (int64_t)pb.N * pb.H * pb.W, pb.C, o.i[0],
                              prm<const float>(params, o.p[0]), reinterpret_cast<const float*>(at(ws, b1.table_off)), b1.C,
                              prm<const float>(params, o.p[1]), reinterpret_cast<const float*>(at(ws, b2.table_off)), b2.C,
                              reinterpret_cast<float*>(at(ws, gb.data_off)), stream);
        break;
      }
      case OP_FINALIZE: {
        if (skip_tables) break;
        const lhn_buf& b = P->bufs[o.out_buf];
        const int src = o.in_buf[0] >= 0 ? o.in_buf[0] : o.out_buf;   // geometry the statistics were taken over
        const lhn_buf& sb = P->bufs[src];
        rc = lhn_bn_finalize(reinterpret_cast<const double*>(at(ws, o.ws[0])), prm<const float>(params, o.p[0]),
                             prm<const float>(params, o.p[1]), prm<float>(params, o.p[2]), prm<float>(params, o.p[3]),
                             prm<int64_t>(params, o.p[4]), reinterpret_cast<float*>(at(ws, b.table_off)), b.C, o.out_coff,
                             o.out_C, reinterpret_cast<float*>(at(ws, o.ws[1])), (double)sb.N * sb.H * sb.W, o.f[0], o.f[1],
                             o.f[2], training, prm<const float>(params, o.p[5]), stream);      // p[5]: bias of the convolution in front, or -1
        break;
      }
      case OP_EW: {
        if (pr && pr[oi] == 2) break;      // ran as job 1 of the op in front
        EwArgs A, B;
        mk_ew_fwd(P, ws, o, &A);
        if (pr && pr[oi] == 1) {
          mk_ew_fwd(P, ws, ops[oi + 1], &B);
          rc = lhn_ew_fwd_pair(&A.job, &B.job, stream);
        } else
          rc = lhn_ew_fwd3(A.srcs, A.job.nsrc, A.job.coef, &A.d, A.job.out_slope, A.job.mode, stream);
        break;
      }
      case OP_MAXPOOL: {
        if (pr && pr[oi] == 2) break;
        MaxpoolArgs A, B;
        mk_maxpool(P, ws, o, false, &A);
        if (pr && pr[oi] == 1) {
          mk_maxpool(P, ws, ops[oi + 1], false, &B);
          rc = lhn_maxpool2_fwd_pair(&A.job, &B.job, stream);
        } else
          rc = lhn_maxpool2_fwd(&A.x, &A.y, stream);
        break;
      }
      case OP_SHUFFLE: {
        lhn_view a = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view b = mkview(P, ws, o.in_buf[1], o.in_coff[1], o.in_C[1]);
        lhn_view d = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        rc = lhn_shuffle2_fwd(&a, &b, &d, stream);
        break;
      }
      case OP_AVGPOOL: {
        if (pr && pr[oi] == 2) break;
        if (pr && pr[oi] == 1) {      // two plain pools (pair_at)
          AvgpoolArgs A, B;
          mk_avgpool(P, ws, o, &A);
          mk_avgpool(P, ws, ops[oi + 1], &B);
          rc = lhn_avgpool_fwd_pair(&A.job, &B.job, stream);
          break;
        }
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0], o.i[2] == 0);
        if (o.ws[1] >= 0 || o.in_buf[1] >= 0) {
          // channel attention: ws[1] = pooling statistics its backward assembles BatchNorm sums from (training plans);
          // in_buf[1] = the pass-through half of a gated unit, copied into the pooled buffer by this launch
          const lhn_bn_slices sl = mkslices(ws, &o.i[5], &o.ws[2], nullptr);
          lhn_view src;
          if (o.in_buf[1] >= 0) src = mkview(P, ws, o.in_buf[1], o.in_coff[1], o.in_C[1]);
          rc = lhn_avgpool_fwd4(&x, reinterpret_cast<float*>(at(ws, o.ws[0])), o.i[0], o.i[1],
                                o.ws[1] >= 0 ? reinterpret_cast<float*>(at(ws, o.ws[1])) : nullptr, &sl, o.in_buf[1] >= 0 ? &src : nullptr, stream);
          break;
        }
        rc = lhn_avgpool_fwd2(&x, reinterpret_cast<float*>(at(ws, o.ws[0])), o.i[0], o.i[1], o.i[3] > 0 ? o.i[3] : x.C, o.i[4], stream);
        break;
      }
      case OP_CA_MLP: {
        const lhn_buf& b = P->bufs[o.out_buf];
        if ((!training || o.ws[3] < 0) && !h0) break;      // not splittable: runs whole on its first half-step
        rc = lhn_ca_mlp_fwd(reinterpret_cast<const float*>(at(ws, o.ws[0])), prm<const float>(params, o.p[0]),
                            prm<const float>(params, o.p[1]), prm<const float>(params, o.p[2]), prm<float>(params, o.p[3]),
                            prm<float>(params, o.p[4]), prm<int64_t>(params, o.p[5]), prm<const float>(params, o.p[6]),
                            prm<const float>(params, o.p[7]), prm<const float>(params, o.p[8]), prm<const float>(params, o.p[9]),
                            (training && o.ws[2] >= 0) ? reinterpret_cast<const float*>(at(ws, o.ws[2])) : nullptr,
                            reinterpret_cast<float*>(at(ws, b.gate_off)), b.C, o.out_coff,
                            reinterpret_cast<float*>(at(ws, o.ws[1])), b.N, o.out_C, o.f[0], o.f[1], training,
                            (training && o.ws[3] >= 0) ? stage : 0, o.ws[3] >= 0 ? reinterpret_cast<double*>(at(ws, o.ws[3])) : nullptr,
                            cscale, stream);
        break;
      }
      case OP_ATT_MLP: {  // p: gamma, beta, rmean, rvar, nbt, w3, b3, wl, bl; ws: pooled, save, mask
        const lhn_buf& b = P->bufs[o.out_buf];
        if ((!training || o.ws[3] < 0) && !h0) break;
        rc = lhn_att_mlp_fwd(reinterpret_cast<const float*>(at(ws, o.ws[0])), prm<const float>(params, o.p[0]),
                             prm<const float>(params, o.p[1]), prm<float>(params, o.p[2]), prm<float>(params, o.p[3]),
                             prm<int64_t>(params, o.p[4]), prm<const float>(params, o.p[5]), prm<const float>(params, o.p[6]),
                             prm<const float>(params, o.p[7]), prm<const float>(params, o.p[8]),
                             (training && o.ws[2] >= 0) ? reinterpret_cast<const float*>(at(ws, o.ws[2])) : nullptr,
                             reinterpret_cast<float*>(at(ws, b.gate_off)), b.C, o.out_coff,
                             reinterpret_cast<float*>(at(ws, o.ws[1])), b.N, o.out_C, o.f[0], o.f[1], training,
                             (training && o.ws[3] >= 0) ? stage : 0, o.ws[3] >= 0 ? reinterpret_cast<double*>(at(ws, o.ws[3])) : nullptr,
                             cscale, stream);
        break;
      }
      case OP_SE_MLP: {  // p: w1, b1, w2, b2; ws: pooled, save; i[0] = J
        const lhn_buf& b = P->bufs[o.out_buf];
        rc = lhn_se_mlp_fwd2(reinterpret_cast<const float*>(at(ws, o.ws[0])), prm<const float>(params, o.p[0]),
                             prm<const float>(params, o.p[1]), prm<const float>(params, o.p[2]), prm<const float>(params, o.p[3]),
                             reinterpret_cast<float*>(at(ws, b.gate_off)), b.C, o.out_coff, reinterpret_cast<float*>(at(ws, o.ws[1])),
                             b.N, o.out_C, o.i[0], o.i[1], stream);
        break;
      }
      // ------------------------------------------------------------------ backward
      case OP_STEM_BWD: {
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        lhn_gradview g = mkgrad(P, ws, o.out_buf, o.i[5] != 0);
        rc = lhn_conv_stem_bwd(static_cast<const float*>(io[0]), &y, &g, prm<float>(grads, o.p[1]), o.i[3], o.i[4], o.i[0],
                               o.i[1], o.i[2], nrep, rstr, stream);
        break;
      }
      case OP_PW_BWD: {
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y;
        lhn_gradview g;
        const float* nchw = nullptr;
        if (o.i[1]) {
          y = x;
          y.data = nullptr; y.table = nullptr; y.gate = nullptr;
          y.cstride = o.out_C; y.coff = 0; y.C = o.out_C;
          g.dz = nullptr; g.dpool = nullptr; g.coef = nullptr;
          nchw = static_cast<const float*>(io[1]);
        } else {
          y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
          g = mkgrad(P, ws, o.out_buf, o.i[5] != 0);
        }
        float* dx = o.i[2] ? reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)) : nullptr;
        lhn_pw_opts po;     // i[3], i[4] = weight rows / columns; i[6], i[7] = stack index / stacks (see OP_PW)
        memset(&po, 0, sizeof(po));
        po.w_rows = o.i[3]; po.w_cols = o.i[4];
        if (nchw && o.i[7] > 1) {
          const int64_t khw = (int64_t)o.out_C * y.H * y.W;
          nchw += (int64_t)o.i[6] * khw;
          po.nchw_batch_stride = (int64_t)o.i[7] * khw;
        }
        const lhn_bnsum bs = mkbns(ws, o.ws[0], o.ws[1], (int)o.f[6], (int)o.f[7]);      // ws[0..1], f[6..7]: the input's producer
        lhn_gatesum gsum;               // the next op's gate-gradient sums ride in this call (see head_gate_fold_at)
        lhn_bn_slices gsl;
        memset(&gsum, 0, sizeof(gsum));
        if (phase == 1 && whole && head_gate_fold_at(P, ops, oi)) {
          const lhn_op& nx = ops[oi + 1];
          gsl = mkslices(ws, &nx.i[0], &nx.ws[5], nullptr);
          gsum.dgate = reinterpret_cast<float*>(at(ws, nx.ws[3]));
          gsum.slices = &gsl;
          gfold_at = oi + 1;
        }
        const int flags = (phase == 1 && whole && P->pw_dz_dead[oi] && !pw_bwd_dy_store()) ? LHN_PW_BWD_DZ_DEAD : 0;
        rc = lhn_conv_pw_bwd6(&x, prm<const float>(params, o.p[0]), &y, &g, dx, o.i[2] == 2, prm<float>(grads, o.p[1]),
                              prm<float>(grads, o.p[2]), o.i[0], nchw, nrep, rstr, &po, bs.sums ? &bs : nullptr,
                              cfin_for == oi ? &cfin : nullptr, gsum.dgate ? &gsum : nullptr, flags, stream);
        break;
      }
      case OP_DW_BWD: {
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        lhn_gradview g = mkgrad(P, ws, o.out_buf, o.i[5] != 0);
        float* dx = o.i[4] ? reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)) : nullptr;
        // ws[4], ws[5] >= 0: BatchNorm-backward sums / saved statistics of the convolution that produced x, i[6] its channel
        // count, i[7] the producer channel of x's first channel (see lhn_conv_dw_bwd2)
        // ws[2], ws[3] >= 0: gradients of residual sums that read x, added to the stored dx (lhn_conv_dw_bwd3)
        // addends win over the sums (which plan.py then leaves to the separate reduce pass); cfin_for == oi: the BatchNorm-backward
        // finalize of y rides in this call (see bwd_fin_consumer)
        const bool adds = o.ws[2] >= 0 || o.ws[3] >= 0;
        const lhn_bnsum bs = mkbns(ws, adds ? -1 : o.ws[4], adds ? -1 : o.ws[5], o.i[6], o.i[7]);
        rc = lhn_conv_dw_bwd4(&x, prm<const float>(params, o.p[0]), &y, &g, dx, o.i[4] == 2, prm<float>(grads, o.p[1]), o.i[0], o.i[1],
                              o.i[2], o.i[3], nrep, rstr, bs.sums ? &bs : nullptr,
                              o.ws[2] >= 0 ? reinterpret_cast<const float*>(at(ws, o.ws[2])) : nullptr,
                              o.ws[3] >= 0 ? reinterpret_cast<const float*>(at(ws, o.ws[3])) : nullptr, cfin_for == oi ? &cfin : nullptr, stream);
        break;
      }
      case OP_KXK_BWD: {
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        lhn_gradview g = mkgrad(P, ws, o.out_buf, o.i[5] != 0);
        float* dx = o.i[2] ? reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)) : nullptr;
        rc = lhn_conv_kxk_bwd(&x, prm<const float>(params, o.p[0]), &y, &g, dx, o.i[2] == 2, prm<float>(grads, o.p[1]), o.i[0],
                              nrep, rstr, o.ws[3] >= 0 ? reinterpret_cast<float*>(at(ws, o.ws[3])) : nullptr, stream);
        break;
      }
      case OP_BN_BWD: {
        const lhn_buf& b = P->bufs[o.out_buf];
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        lhn_gradview g = mkgrad(P, ws, o.out_buf, false);
        double* sums = reinterpret_cast<double*>(at(ws, o.ws[0]));
        const float* save = reinterpret_cast<const float*>(at(ws, o.ws[1]));
        lhn_bnbwdfin fin;
        fin.counter = reinterpret_cast<uint32_t*>(at(ws, o.ws[2]));
        fin.gamma = prm<const float>(params, o.p[0]);
        fin.coef = reinterpret_cast<float*>(at(ws, b.coef_off));
        fin.dgamma = prm<float>(grads, o.p[1]);
        fin.dbeta = prm<float>(grads, o.p[2]);
        fin.count = (double)b.N * b.H * b.W * cscale;
        fin.cstride = b.C; fin.coff = o.out_coff; fin.C = o.out_C;
        if (fin.counter && fuse_finalize() && whole && !o.i[1]) {
          rc = lhn_bn_bwd_reduce(&y, &g, save, sums, &fin, stream);
        } else {
          if (h0 && !o.i[1]) rc = lhn_bn_bwd_reduce(&y, &g, save, sums, nullptr, stream);      // i[1]: sums come from the reader's backward
          // consumer-side finalize: the next op is the backward of the convolution that owns this BatchNorm and reads coef
          const lhn_op* nx = oi + 1 < ops.size() ? &ops[oi + 1] : nullptr;
          if (!rc && h1 && whole && bwd_fin_consumer() && !fuse_finalize() && o.i[0] == 0 && nx &&
              (nx->kind == OP_DW_BWD || (nx->kind == OP_PW_BWD && !nx->i[1])) && nx->out_buf == o.out_buf && nx->out_coff == o.out_coff &&
              nx->out_C == o.out_C && nx->i[5] != 0) {
            cfin.sums = sums;
            cfin.save_mean_invstd = save;
            cfin.gamma = fin.gamma;
            cfin.dgamma = fin.dgamma;
            cfin.dbeta = fin.dbeta;
            cfin.count = fin.count;
            cfin.pgrad_scale = pscale;
            cfin.stat_channels = o.out_C;
            cfin_for = oi + 1;
          } else if (!rc && h1)
            rc = lhn_bn_bwd_finalize2(sums, fin.gamma, save, fin.coef, b.C, o.out_coff, o.i[0] > 0 ? o.i[0] : o.out_C, o.out_C, fin.count,
                                      fin.dgamma, fin.dbeta, pscale, stream);      // i[0]: real channels of a padded output
        }
        break;
      }
      case OP_EW_BWD: {
        if (pr && pr[oi] == 2) break;
        if (pr && pr[oi] == 1) {      // two sums of one form (pair_at)
          EwArgs A, B;
          mk_ew_bwd(P, ws, o, &A);
          mk_ew_bwd(P, ws, ops[oi + 1], &B);
          rc = o.i[1] == 3 ? lhn_ew_bwd_multi_pair(&A.job, &B.job, stream) : lhn_ew_bwd_pair(&A.job, &B.job, stream);
          break;
        }
        lhn_view src = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view d = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        const lhn_buf& db = P->bufs[o.out_buf];
        if (o.i[1] == 1) {            // product: in_buf[1] = the other operand
          lhn_view other = mkview(P, ws, o.in_buf[1], o.in_coff[1], o.in_C[1]);
          rc = lhn_ew_mul_bwd(&src, &other, &d, reinterpret_cast<const float*>(at(ws, db.grad_off)),
                              reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)), o.i[0], stream);
        } else if (o.i[1] == 2) {     // bilinearly resampled source
          rc = lhn_bilinear_bwd(&src, &d, reinterpret_cast<const float*>(at(ws, db.grad_off)),
                                reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)), o.i[0], o.f[0], stream);
        } else if (o.i[1] == 3) {     // 2 or 3 sources of the destination's resolution in one pass: in_buf[0..2]; accumulate flags i[0], i[2],
                                      // i[3]; their producers' sums ws[0..5], (C, coff) in i[4..7] and f[4..5]
          lhn_view srcs[3];
          float* dsrcs[3];
          int acc[3] = {o.i[0], o.i[2], o.i[3]};
          lhn_bnsum bsv[3] = {mkbns(ws, o.ws[0], o.ws[1], o.i[4], o.i[5]), mkbns(ws, o.ws[2], o.ws[3], o.i[6], o.i[7]),
                              mkbns(ws, o.ws[4], o.ws[5], (int)o.f[4], (int)o.f[5])};
          const lhn_bnsum* bsp[3];
          int ns = 0;
          for (; ns < 3 && o.in_buf[ns] >= 0; ++ns) {
            srcs[ns] = mkview(P, ws, o.in_buf[ns], o.in_coff[ns], o.in_C[ns]);
            dsrcs[ns] = reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[ns]].grad_off));
            bsp[ns] = bsv[ns].sums ? &bsv[ns] : nullptr;
          }
          rc = lhn_ew_bwd_multi(srcs, ns, &d, reinterpret_cast<const float*>(at(ws, db.grad_off)),
                                reinterpret_cast<const float*>(at(ws, db.dpool_off)), o.f[0], dsrcs, acc, bsp, stream);
        } else {
          const lhn_bnsum bs = mkbns(ws, o.ws[0], o.ws[1], o.i[4], o.i[5]);
          rc = lhn_ew_bwd3(&src, &d, reinterpret_cast<const float*>(at(ws, db.grad_off)),
                           reinterpret_cast<const float*>(at(ws, db.dpool_off)), o.f[0],
                           reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)), o.i[0], bs.sums ? &bs : nullptr, stream);
        }
        break;
      }
      case OP_MAXPOOL_BWD: {
        if (pr && pr[oi] == 2) break;
        MaxpoolArgs A, B;
        mk_maxpool(P, ws, o, true, &A);
        if (pr && pr[oi] == 1) {
          mk_maxpool(P, ws, ops[oi + 1], true, &B);
          rc = lhn_maxpool2_bwd_pair(&A.job, &B.job, stream);
        } else
          rc = lhn_maxpool2_bwd3(&A.x, &A.y, A.job.dy, A.job.dx, A.job.dx_accumulate, A.job.bns, A.job.adds, stream);
        break;
      }
      case OP_AVGPOOL_BWD: {
        lhn_view x = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        const lhn_bnsum bs = mkbns(ws, o.ws[1], o.ws[2], o.i[5], o.i[6]);
        rc = lhn_avgpool_bwd3(&x, reinterpret_cast<const float*>(at(ws, o.ws[0])), o.i[0], o.i[1], o.i[3] > 0 ? o.i[3] : x.C, o.i[4],
                              reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)), o.i[2], bs.sums ? &bs : nullptr, stream);
        break;
      }
      case OP_SHUFFLE_BWD: {     // i[0], i[1]: 0 = no gradient wanted, 1 = store, 2 = accumulate (operand a, b)
        lhn_view a = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]);
        lhn_view b = mkview(P, ws, o.in_buf[1], o.in_coff[1], o.in_C[1]);
        lhn_view d = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        rc = lhn_shuffle2_bwd(&a, &b, &d, reinterpret_cast<const float*>(at(ws, P->bufs[o.out_buf].grad_off)),
                              o.i[0] ? reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)) : nullptr, o.i[0] == 2,
                              o.i[1] ? reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[1]].grad_off)) : nullptr, o.i[1] == 2, stream);
        break;
      }
      case OP_GATE_REDUCE: {
        if (gfold_at == oi) break;      // dgate | T0 | T1 are in the arena already
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C, false);
        float* dg = reinterpret_cast<float*>(at(ws, o.ws[3]));
        const lhn_bn_slices sl = mkslices(ws, &o.i[0], &o.ws[5], nullptr);
        // (dgate lives in the arena the backward zeroes with one memset: prezeroed)
        rc = lhn_gate_bwd_reduce3(&y, reinterpret_cast<const float*>(at(ws, P->bufs[o.out_buf].grad_off)), dg,
                                  o.ws[4] >= 0 ? dg + (size_t)y.N * y.C : nullptr, &sl, 1, stream);
        break;
      }
      case OP_CA_MLP_BWD: {
        const lhn_buf& b = P->bufs[o.out_buf];
        if (o.ws[4] < 0 && !h0) break;
        const lhn_bn_slices sl = mkslices(ws, &o.i[0], &o.ws[6], &o.ws[8]);
        const float* dgp = reinterpret_cast<const float*>(at(ws, o.ws[3]));
        rc = lhn_ca_mlp_bwd2(reinterpret_cast<const float*>(at(ws, o.ws[0])), prm<const float>(params, o.p[0]),
                            prm<const float>(params, o.p[1]), prm<const float>(params, o.p[2]), prm<const float>(params, o.p[3]),
                            o.ws[2] >= 0 ? reinterpret_cast<const float*>(at(ws, o.ws[2])) : nullptr,
                            reinterpret_cast<const float*>(at(ws, o.ws[1])), reinterpret_cast<const float*>(at(ws, o.ws[3])),
                            reinterpret_cast<float*>(at(ws, b.dpool_off)), b.C, o.out_coff, b.H, b.W, prm<float>(grads, o.p[4]),
                            prm<float>(grads, o.p[5]), prm<float>(grads, o.p[6]), prm<float>(grads, o.p[7]),
                            prm<float>(grads, o.p[8]), prm<float>(grads, o.p[9]), prm<float>(grads, o.p[10]), b.N, o.out_C,
                            o.ws[4] >= 0 ? stage : 0, o.ws[4] >= 0 ? reinterpret_cast<double*>(at(ws, o.ws[4])) : nullptr, cscale, pscale,
                            o.ws[5] >= 0 ? dgp + (size_t)b.N * b.C : nullptr, o.ws[5] >= 0 ? reinterpret_cast<const float*>(at(ws, o.ws[5])) : nullptr,
                            &sl, stream);
        break;
      }
      case OP_ATT_MLP_BWD: {  // p: gamma, beta, w3, wl (params) | dgamma, dbeta, dw3, db3, dwl, dbl (grads); ws: pooled, save, mask, dgate
        const lhn_buf& b = P->bufs[o.out_buf];
        if (o.ws[4] < 0 && !h0) break;
        rc = lhn_att_mlp_bwd(reinterpret_cast<const float*>(at(ws, o.ws[0])), prm<const float>(params, o.p[0]),
                             prm<const float>(params, o.p[1]), prm<const float>(params, o.p[2]), prm<const float>(params, o.p[3]),
                             o.ws[2] >= 0 ? reinterpret_cast<const float*>(at(ws, o.ws[2])) : nullptr,
                             reinterpret_cast<float*>(at(ws, o.ws[1])), reinterpret_cast<const float*>(at(ws, o.ws[3])),
                             reinterpret_cast<float*>(at(ws, b.dpool_off)), b.C, o.out_coff, b.H, b.W, prm<float>(grads, o.p[4]),
                             prm<float>(grads, o.p[5]), prm<float>(grads, o.p[6]), prm<float>(grads, o.p[7]),
                             prm<float>(grads, o.p[8]), prm<float>(grads, o.p[9]), b.N, o.out_C,
                             o.ws[4] >= 0 ? stage : 0, o.ws[4] >= 0 ? reinterpret_cast<double*>(at(ws, o.ws[4])) : nullptr, cscale, pscale,
                             stream);
        break;
      }
      case OP_SE_MLP_BWD: {  // p: w1, w2 (params) | dw1, db1, dw2, db2 (grads); ws: pooled, save, -, dgate; i[0] = J
        const lhn_buf& b = P->bufs[o.out_buf];
        rc = lhn_se_mlp_bwd2(reinterpret_cast<const float*>(at(ws, o.ws[0])), prm<const float>(params, o.p[0]),
                             prm<const float>(params, o.p[1]), reinterpret_cast<const float*>(at(ws, o.ws[1])),
                             reinterpret_cast<const float*>(at(ws, o.ws[3])), reinterpret_cast<float*>(at(ws, b.dpool_off)), b.C,
                             o.out_coff, b.H, b.W, prm<float>(grads, o.p[2]), prm<float>(grads, o.p[3]), prm<float>(grads, o.p[4]),
                             prm<float>(grads, o.p[5]), b.N, o.out_C, o.i[0], o.i[1], stream);
        break;
      }
      case OP_CBAM: {  // in: p, r; p: w1, w2, w7; ws: save
        lhn_view p = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]), r = mkview(P, ws, o.in_buf[1], o.in_coff[1], o.in_C[1]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        rc = lhn_cbam_fwd(&p, &r, prm<const float>(params, o.p[0]), prm<const float>(params, o.p[1]), prm<const float>(params, o.p[2]),
                          &y, reinterpret_cast<float*>(at(ws, o.ws[0])), stream);
        break;
      }
      case OP_CBAM_BWD: {  // in: p, r; p: w1, w2, w7 (params) | dw1, dw2, dw7 (grads); ws: save, scratch
        lhn_view p = mkview(P, ws, o.in_buf[0], o.in_coff[0], o.in_C[0]), r = mkview(P, ws, o.in_buf[1], o.in_coff[1], o.in_C[1]);
        lhn_view y = mkview(P, ws, o.out_buf, o.out_coff, o.out_C);
        rc = lhn_cbam_bwd(&p, &r, prm<const float>(params, o.p[0]), prm<const float>(params, o.p[1]), prm<const float>(params, o.p[2]),
                          &y, reinterpret_cast<const float*>(at(ws, P->bufs[o.out_buf].grad_off)),
                          reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[0]].grad_off)),
                          reinterpret_cast<float*>(at(ws, P->bufs[o.in_buf[1]].grad_off)), prm<float>(grads, o.p[3]),
                          prm<float>(grads, o.p[4]), prm<float>(grads, o.p[5]), reinterpret_cast<const float*>(at(ws, o.ws[0])),
                          reinterpret_cast<float*>(at(ws, o.ws[1])), stream);
        break;
      }
      default:
        lhn_set_error("lhn_plan_run: unknown op kind %d at index %zu", o.kind, oi);
        rc = 1;
    }
  }
  return rc;
}

// SyncBatchNorm driver entry: run the half-steps [step_begin, step_end) of a phase (see run_ops).  The caller all-reduces
// the statistics buffer of op i between step 2*i and step 2*i+1.
int lhn_plan_run_range(void* plan, int phase, int64_t step_begin, int64_t step_end, void* ws, void* const* params,
                       void* const* grads, void* const* io, int training, int grad_replicas, int64_t grad_rep_stride,
                       double count_scale, float pgrad_scale, void* stream) {
  LHN_CHECK_ARG(plan && ws && params && io && step_begin >= 0 && step_end >= step_begin && count_scale >= 1, "lhn_plan_run_range: bad argument");
  LHN_CHECK_ARG(phase == 0 || (phase == 1 && grads), "lhn_plan_run_range: phase %d", phase);
  return run_ops(static_cast<const Plan*>(plan), phase, ws, params, grads, io, training, grad_replicas < 1 ? 1 : grad_replicas,
                 grad_rep_stride, stream, (size_t)step_begin, (size_t)step_end, count_scale, pgrad_scale);
}

static bool graphs_enabled() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("LHN_GRAPH");
    v = (e && e[0] == '1') ? 1 : 0;
  }
  return v == 1;
}
static uint64_t hash_ptrs(void* const* a, const std::vector<lhn_op>& ops, bool grads) {
  // only the entries the ops reference (p[] indices) matter; FNV-1a over their values
  uint64_t h = 1469598103934665603ull;
  if (!a) return h;
  for (const lhn_op& o : ops)
    for (int k = 0; k < 12; ++k)
      if (o.p[k] >= 0) {
        h ^= reinterpret_cast<uint64_t>(a[o.p[k]]);
        h *= 1099511628211ull;
      }
  (void)grads;
  return h;
}

// Runs one phase.  With LHN_RUN_GRAPH in `training` (or LHN_GRAPH=1 in the environment) the launch sequence of a (phase, pointer set) is captured into a hipGraph the second
// time it is seen and replayed afterwards (one graph launch instead of 150-400 kernel launches: the small-batch /
// low-resolution end of the network is launch-bound).  The plan is static, so a graph is valid for as long as the
// workspace, parameter, gradient and io pointers repeat; a different pointer set simply gets its own graph (LRU of 8),
// and a plan whose pointers never repeat falls back to plain launches.
int lhn_plan_run(void* plan, int phase, void* ws, void* const* params, void* const* grads, void* const* io, int training,
                 int grad_replicas, int64_t grad_rep_stride, void* stream) {
  const int nrep = grad_replicas < 1 ? 1 : grad_replicas;
  const int64_t rstr = grad_rep_stride;
  LHN_CHECK_ARG(plan && ws && params && io, "lhn_plan_run: null argument");
  LHN_CHECK_ARG(phase == 0 || (phase == 1 && grads), "lhn_plan_run: phase %d", phase);
  Plan* P = static_cast<Plan*>(plan);
  // (the legacy default stream cannot be captured: graphs need the caller to run on a real stream)
  const bool want_graph = graphs_enabled() || (training & LHN_RUN_GRAPH) != 0;
  training &= ~LHN_RUN_GRAPH;
  if (!want_graph || stream == nullptr || P->graph_misses > 64) return run_ops(P, phase, ws, params, grads, io, training, nrep, rstr, stream);
  const std::vector<lhn_op>& ops = phase == 0 ? P->fwd : P->bwd;
  const uint64_t ph = hash_ptrs(params, ops, false), gh = phase == 1 ? hash_ptrs(grads, ops, true) : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  GraphEntry* e = nullptr;
  for (GraphEntry& g : P->graphs)
    if (g.phase == phase && g.training == training && g.nrep == nrep && g.rstr == rstr && g.ws == ws && g.io0 == io[0] &&
        g.io1 == io[1] && g.phash == ph && g.ghash == gh) {
      e = &g;
      break;
    }
  ++P->tick;
  if (e && e->exec) {
    e->last_use = P->tick;
    if (hipGraphLaunch(e->exec, s) != hipSuccess) {
      lhn_set_error("lhn_plan_run: hipGraphLaunch failed");
      return 2;
    }
    return 0;
  }
  if (!e) {  // first sighting: run eagerly (also initialises every kernel's one-time attributes), remember the key
    ++P->graph_misses;
    if (P->graphs.size() >= 8) {
      size_t victim = 0;
      for (size_t i = 1; i < P->graphs.size(); ++i)
        if (P->graphs[i].last_use < P->graphs[victim].last_use) victim = i;
      if (P->graphs[victim].exec) (void)hipGraphExecDestroy(P->graphs[victim].exec);
      P->graphs.erase(P->graphs.begin() + victim);
    }
    P->graphs.push_back(GraphEntry{phase, training, nrep, 1, rstr, ws, io[0], io[1], ph, gh, nullptr, P->tick});
    return run_ops(P, phase, ws, params, grads, io, training, nrep, rstr, stream);
  }
  // second sighting: capture, instantiate, launch
  e->last_use = P->tick;
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess)
    return run_ops(P, phase, ws, params, grads, io, training, nrep, rstr, stream);
  const int rc = run_ops(P, phase, ws, params, grads, io, training, nrep, rstr, stream);
  const hipError_t ec = hipStreamEndCapture(s, &graph);
  if (rc != 0 || ec != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();
    P->graph_misses = 1000;     // capture is not possible here: stay on plain launches
    return rc != 0 ? rc : run_ops(P, phase, ws, params, grads, io, training, nrep, rstr, stream);
  }
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess || !exec) {
    (void)hipGetLastError();
    P->graph_misses = 1000;
    return run_ops(P, phase, ws, params, grads, io, training, nrep, rstr, stream);
  }
  e->exec = exec;
  P->graph_misses = 0;
  if (hipGraphLaunch(exec, s) != hipSuccess) {
    lhn_set_error("lhn_plan_run: hipGraphLaunch failed");
    return 2;
  }
  return 0;
}
}  // extern "C"
