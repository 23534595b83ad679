/* liblhn -- MI355X (gfx950) kernels for litehandnet's convolutional heatmap path.
 *
 * C ABI only: raw device pointers, explicit sizes, a hipStream_t (passed as void*), int status.
 * 0 = ok; nonzero = invalid argument / unsupported shape / HIP error, text via lhn_last_error().
 * Nothing here allocates or frees caller memory; every tensor is borrowed for the duration of
 * the call on the given stream.  The reference has no native interface -- each entry point cites
 * the Python function (file:line under the reference tree) whose arithmetic it replaces.
 *
 * Activation layout inside the library: NHWC fp32.  A buffer may carry a *pending* per-channel
 * transform (BatchNorm scale/shift + leaky slope, written by lhn_bn_finalize) and a per-(n,c)
 * gate (channel attention); consumers apply   v = gate[n,c] * lrelu_slope[c](scale[c]*raw+shift[c])
 * on load, so train-mode BatchNorm costs no extra pass over HBM.
 */
#ifndef LHN_H
#define LHN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LHN_VERSION 3
/* cross-block accumulators (BN statistics, BN-backward sums) are replicated to spread atomic traffic:
 * layout double[LHN_STAT_REPLICAS][2][C]; a block adds into replica (blockIdx % LHN_STAT_REPLICAS). */
#define LHN_STAT_REPLICAS 32

typedef struct lhn_view {
  float*       data;    /* base of the [N,H,W,cstride] buffer                                        */
  const float* table;   /* [3][cstride] scale | shift | slope, absolute channel index; NULL=identity */
  const float* gate;    /* [N][cstride] or NULL                                                      */
  int32_t N, H, W;
  int32_t cstride;      /* channels of the underlying buffer                                          */
  int32_t coff;         /* first channel of the view                                                  */
  int32_t C;            /* channels of the view                                                       */
  const void* pend;      /* reserved, must be NULL (round 2's deferred BatchNorm finalize is gone; the field keeps the layout) */
} lhn_view;

/* gradient-side companion of a BatchNorm'd conv output (see DESIGN.md "backward") */
typedef struct lhn_gradview {
  const float* dz;       /* gradient w.r.t. the consumed value z, same geometry as the forward view  */
  const float* dpool;    /* [N][25][cstride] channel-attention pooled gradient per bin-overlap segment
                          * (sum over the segment's bins of d(loss)/d(pooled)/|bin|), or NULL          */
  const float* coef;     /* [3][cstride]  A | B | C :  dy = A*du + B*y + C   (NULL: dy = du)          */
} lhn_gradview;

/* Optional fused BatchNorm finalize: the last workgroup of the conv launch to finish folds the replicated
 * statistics into the table (same arithmetic as lhn_bn_finalize) -- saves one launch per BatchNorm.
 * `counter` must be zero before the launch.  NULL pointer to the struct = not fused. */
typedef struct lhn_bnfin {
  uint32_t*    counter;
  const float* gamma;
  const float* beta;
  float*       running_mean;
  float*       running_var;
  int64_t*     num_batches_tracked;
  float*       table;
  float*       save_mean_invstd;
  double       count;
  int32_t      cstride, coff, C;
  float        eps, momentum, slope;
  const float* conv_bias;   /* bias of the convolution in front of the BatchNorm, or NULL (see lhn_bn_finalize) */
} lhn_bnfin;
/* same idea for lhn_bn_bwd_reduce -> lhn_bn_bwd_finalize.  The slice must be y's: cstride, coff and C equal to those of the view
 * the reduction runs over (the kernel strides sums and save by y->C), anything else returns the invalid-argument status before
 * the launch.  The fused form has no pgrad_scale (dgamma / dbeta get the plain sums): SyncBatchNorm runs, which scale them by
 * 1 / world, take the separate lhn_bn_bwd_finalize launch. */
typedef struct lhn_bnbwdfin {
  uint32_t*    counter;
  const float* gamma;
  float*       coef;
  float*       dgamma;
  float*       dbeta;
  double       count;
  int32_t      cstride, coff, C;
} lhn_bnbwdfin;

/* BatchNorm-backward finalize on the CONSUMER side.  The (A, B, C) coefficients of  dy = A*du + B*y + C  are read by one kernel only:
 * the backward of the convolution that owns the BatchNorm (y of that call).  lhn_conv_dw_bwd4 / lhn_conv_pw_bwd4 take the finished
 * sums instead of a finalized gy->coef: every workgroup folds the replicas of its own channels in its prologue (the order and the
 * double arithmetic of lhn_bn_bwd_finalize2: same sums, same bits), and one workgroup per channel also stores coef (into gy->coef
 * at y's cstride / coff) and adds dgamma / dbeta -- memory holds what the separate launch leaves.  The BatchNorm has y->C channels.
 * Where the launcher picks a kernel without the in-prologue fold it calls lhn_bn_bwd_finalize2 itself first: the result never
 * depends on the kernel chosen.  NULL pointer to the struct (or sums == NULL): gy->coef is read as it is. */
typedef struct lhn_bnbwdsrc {
  const double* sums;              /* [LHN_STAT_REPLICAS][2][stat_channels]: sum du | sum du * xhat, complete before the call */
  const float*  save_mean_invstd;  /* [2][stat_channels]                                                                     */
  const float*  gamma;             /* [C] or NULL (= 1)                                                                       */
  float*        dgamma;            /* [C] added to, or NULL                                                                   */
  float*        dbeta;             /* [C] added to, or NULL                                                                   */
  double        count;             /* N*H*W (times the world size under SyncBatchNorm)                                        */
  float         pgrad_scale;       /* as lhn_bn_bwd_finalize                                                                  */
  int32_t       stat_channels;     /* channel stride of sums / save, >= y->C                                                  */
} lhn_bnbwdsrc;

/* BatchNorm FORWARD finalize on the consumer side.  The table (scale | shift | slope) of a convolution + BatchNorm output is read
 * first by the next kernel; when that kernel is a depthwise or 1x1 convolution over exactly the BatchNorm's channels,
 * lhn_conv_dw_fwd4 / lhn_conv_pw_fwd3 take the finished statistics instead of a finalized x->table: every workgroup folds the
 * replicas of its own input channels in its prologue, while its first tile's loads are in flight (replica order and double arithmetic of
 * lhn_bn_finalize: same sums, same bits), and one workgroup per channel also stores the table slice, mean | invstd, one momentum
 * step of the running statistics and num_batches_tracked + 1 -- memory holds what the separate launch leaves, for every later
 * reader.  The slice must be x's: table == x->table, cstride / coff / C equal to the view's.  Where the launcher picks a kernel
 * without the in-prologue fold it calls lhn_bn_finalize itself first: the result never depends on the kernel chosen.  NULL pointer
 * to the struct (or stats == NULL): x->table is read as it is. */
typedef struct lhn_bnfinsrc {
  const double* stats;              /* [LHN_STAT_REPLICAS][2][C]: sum | sum of squares, complete before the call               */
  const float*  gamma;              /* [C] or NULL (= 1)                                                                       */
  const float*  beta;               /* [C] or NULL (= 0)                                                                       */
  const float*  conv_bias;          /* bias of the convolution in front of the BatchNorm, or NULL (see lhn_bn_finalize)        */
  float*        running_mean;       /* [C] or NULL (then running_var is not touched either)                                    */
  float*        running_var;
  int64_t*      num_batches_tracked;/* or NULL                                                                                 */
  float*        table;              /* base of the [3][cstride] table: the slice [coff, coff + C) of each row is written       */
  float*        save_mean_invstd;   /* [2][C] or NULL                                                                          */
  double        count;              /* N*H*W of the BatchNorm (times the world size under SyncBatchNorm)                       */
  int32_t       cstride, coff, C;
  float         eps, momentum, slope;
} lhn_bnfinsrc;

/* BatchNorm-backward sums contributed by a READER. du = dz * act'(u) is linear in dz, and dz of a convolution output is the sum
 * of what its readers' backward kernels hand back -- so every reader that has its own part of dz in registers can add that
 * part's  sum du  and  sum du * xhat  into the PRODUCER's replicated sums (the reader holds the raw value and the table of its
 * input anyway, or re-reads a tile that is still in L2).  When all readers of a convolution + BatchNorm output do, its
 * lhn_bn_bwd_reduce pass (one read of y and one of dz) is not needed.  Valid for ungated inputs without pooled gradient.
 *   sums: [LHN_STAT_REPLICAS][2][C] of the producer's BatchNorm (zeroed by the caller), save: its [2][C] mean | invstd,
 *   coff: the channel of that BatchNorm which the reader's input view starts at.  NULL pointer to the struct: no sums. */
typedef struct lhn_bnsum {
  double*      sums;
  const float* save;
  int32_t      C, coff;
} lhn_bnsum;
/* Gradient contributions of OTHER readers of x that join the store of lhn_maxpool2_bwd3 (the hourglass skip tensor is read by
 * a 2x2 max-pool, an adaptive average pool and a plain sum: litehourglass.py:139-163, pose_hg_ms_att.py -- three read-modify-write
 * passes over its gradient otherwise).  same: gradient of a sum that reads x at its own resolution with coefficient 1 and no
 * activation behind it (x's geometry); pooled: gradient of adaptive_avg_pool2d(x, (OH, OW)) as [N][OH][OW][pooled_cstride].
 * Either may be NULL.  x.H and x.W must be even (every pixel of x sits in one pooling window). */
typedef struct lhn_grad_adds {
  const float* same;
  int32_t      same_cstride, same_coff;
  const float* pooled;
  int32_t      OH, OW, pooled_cstride, pooled_coff;
} lhn_grad_adds;

int         lhn_version(void);
/* 1 when the library runs in its deterministic mode (environment LHN_DETERMINISTIC=1, read once): every cross-workgroup sum
 * has one writer per replica and replicas are folded in a fixed order, so two runs on the same inputs agree bit for bit
 * (forward, gradients, running statistics).  Grids shrink to at most 16 workgroups: expect a 20-40x slower step. */
int         lhn_deterministic(void);
const char* lhn_last_error(void);
int         lhn_device_ok(void);              /* 0 if a gfx950 device is usable                       */

/* ---------------------------------------------------------------- heatmap encode / decode / loss
 * lhn_heatmap_encode    datasets/data_pipeline/generateTarget.py:74-159 (_msra_generate_target)
 * lhn_heatmap_argmax    utils/post_processing/evaluation/top_down_eval.py:199-231 (_get_max_preds)
 * lhn_heatmap_refine    .../top_down_eval.py:440-452 ('default' +-0.25 shift); mode 1 =
 *                       utils/heatmap_post_processing.py:6-33 / utils/HeatmapParser.py:197-223 twin; a mode-1 coordinate
 *                       outside the map (the (-1, -1) of a map without a positive maximum) reads nothing: both shifts -0.25
 * lhn_transform_preds   datasets/data_pipeline/post_transforms.py:6-48
 * lhn_heatmap_decode    .../top_down_eval.py:375-463 (keypoints_from_heatmaps, 'default'), fused
 * lhn_heatmap_nms       utils/HeatmapParser.py:41-50 (k x k max-pool peak keep)
 * lhn_pck_accuracy      .../top_down_eval.py:12-62,129-165
 * lhn_eval_*            datasets/datasets/base_dataset.py:193-261 (_report_metric: PCK, AUC, EPE over the whole test set)
 * lhn_loss_balanced_mse loss/loss.py:93-114 + loss/heatmapLoss.py:242-265
 */
int lhn_heatmap_encode(const float* joints /*[N,K,3]*/, const float* visible /*[N,K,3]*/,
                       float* target /*[N,K,H,W]*/, float* weight /*[N,K]*/, int N, int K, int H, int W,
                       float img_w, float img_h, float sigma, int unbiased /*0 MSRA patch, 1 DARK full map, 2 UDP patch (generateTarget.py:160-236)*/,
                       void* stream);
int lhn_heatmap_argmax(const float* hm /*[N,K,H,W]*/, float* preds /*[N,K,2]*/, float* maxvals /*[N,K]*/,
                       int32_t* index /*[N,K] or NULL*/, int N, int K, int H, int W, void* stream);
int lhn_heatmap_refine(const float* hm, float* preds /*[N,K,2] in/out*/, int N, int K, int H, int W,
                       int mode, void* stream);
int lhn_transform_preds(const float* coords /*[N,K,2]*/, const float* center /*[N,2]*/,
                        const float* scale /*[N,2]*/, float* out /*[N,K,2]*/, int N, int K, int W, int H,
                        int use_udp, void* stream);
int lhn_heatmap_decode(const float* hm, const float* center, const float* scale, float* hm_preds,
                       float* preds, float* maxvals, int N, int K, int H, int W, int post_process,
                       void* stream);
/* GPU input path: TopDownAffine (datasets/data_pipeline/topdown_affine.py:47-114, non-UDP) +
 * ToTensor + NormalizeTensor (shared_transform.py:3-44) in one launch: uint8 HWC source images [N,Hs,Ws,3] -> normalised
 * float CHW crops [N,3,Ho,Wo]; optionally maps joints [N,K,3] (visible ones) with the same transform.  mean3/std3 are
 * HOST pointers to 3 floats.  cv2.warpAffine parity is unpinned (cv2 absent): exact-float bilinear, uint8 rounding. */
int lhn_affine_warp_normalize(const unsigned char* img, int N, int Hs, int Ws, const float* center /*[N,2]*/,
                              const float* scale /*[N,2]*/, const float* rot_deg /*[N]*/, const float* mean3,
                              const float* std3, float* out, int Ho, int Wo, float* joints /*or NULL*/,
                              const float* visible, int vis_stride, int K,
                              int use_udp /*get_warp_matrix + warp_affine_joints, post_transforms.py:49-100*/, void* stream);
/* TopDownRandomFlip (datasets/data_pipeline/RandomFlip.py:28-100) for the samples with flipped[n] != 0: lhn_random_flip
 * exchanges the joints / visibility of every (left, right) pair, mirrors x (W - 1 - x), multiplies by the visibility and
 * mirrors center_x; lhn_affine_warp_normalize2 then reads the source image of those samples mirrored (img[:, ::-1]) --
 * the flipped image is never written.  pairs: int32 [npairs][2] on the device. */
/* HSVRandomAug (datasets/data_pipeline/random_hsv.py:20-34) in place on uint8 BGR images [N,H,W,3]: gains = int16 [N][3] (hue,
 * saturation, value), drawn by the caller exactly as the reference draws them (litehandnet_amd.pipeline.hsv_gains).  The integer
 * jitter is the reference's; the 8-bit colour conversions follow OpenCV's algorithm (cv2 absent here: parity unpinned). */
int lhn_hsv_jitter(unsigned char* img, const int16_t* gains, int N, int H, int W, void* stream);
int lhn_random_flip(float* joints /*[N,K,3]*/, float* visible /*[N,K,vis_stride]*/, int vis_stride, float* center /*[N,2]*/,
                    const unsigned char* flipped /*[N]*/, const int32_t* pairs, int npairs, int N, int K, int img_width,
                    void* stream);
int lhn_affine_warp_normalize2(const unsigned char* img, int N, int Hs, int Ws, const float* center, const float* scale,
                               const float* rot_deg, const float* mean3, const float* std3, float* out, int Ho, int Wo,
                               float* joints, const float* visible, int vis_stride, int K, int use_udp,
                               const unsigned char* flipped /*[N] or NULL*/, void* stream);
/* SimDR (cfg.PIPELINE.simdr_split_ratio = k > 0): 1-D Gaussian target vectors (generate_simder.py:9-31) and the
 * auxiliary loss on the decoded vectors (centernet_simdr_loss.py:6-71: per joint, SmoothL1 'mean' over [N, L] times the
 * MEAN of that joint's weights, x and y, averaged over joints).  The two shared Linear decoders are plain library
 * GEMMs on the caller's side; decoding the vectors is lhn_heatmap_argmax on [N,K,1,L] + lhn_transform_preds.
 * sums = double[3*K] scratch shared by fwd and bwd. */
int lhn_simdr_encode(const float* joints /*[N,K,3]*/, const float* visible, int vis_stride, float* target_x /*[N,K,Wd]*/,
                     float* target_y /*[N,K,Hd]*/, int N, int K, int Wd, int Hd, float k, float sigma, void* stream);
int lhn_simdr_loss_fwd(const float* px, const float* py, const float* tx, const float* ty, const float* weight /*[N,K]*/,
                       double* sums, float* loss, int N, int K, int Wd, int Hd, void* stream);
int lhn_simdr_loss_bwd(const float* px, const float* py, const float* tx, const float* ty, const double* sums,
                       const float* gout, float* dpx, float* dpy, int N, int K, int Wd, int Hd, void* stream);
/* DARK 'unbiased' decode: k x k Gaussian modulation + log + Taylor step (top_down_eval.py:233-272,338-372,433-439;
 * twin utils/heatmap_post_processing.py:35-91), fused with argmax and transform_preds */
int lhn_heatmap_decode_dark(const float* hm, const float* center, const float* scale, float* hm_preds,
                            float* preds, float* maxvals, int N, int K, int H, int W, int kernel, void* stream);
/* UDP + DARK decode: keypoints_from_heatmaps(use_udp=True, GaussianHeatmap) = _get_max_preds + post_dark_udp
 * (top_down_eval.py:275-337, 404-411) + transform_preds(use_udp=True) (post_transforms.py:37-43) */
int lhn_heatmap_decode_dark_udp(const float* hm, const float* center, const float* scale, float* hm_preds,
                                float* preds, float* maxvals, int N, int K, int H, int W, int kernel, void* stream);
int lhn_heatmap_nms(float* hm /*in place*/, float* scratch /*same size*/, int N, int K, int H, int W,
                    int kernel, void* stream);
/* HeatmapParser.candidate_bbox (utils/HeatmapParser.py:52-85): per centre map [N,H,W] (after lhn_heatmap_nms) the k highest
 * peaks in descending order as candidates[N,k,5] = (x, y, w, h, confidence) in image pixels; size_maps [N,2,H,W] = the
 * region-averaged width / height ratio maps (NULL: w = h = 0). */
int lhn_heatmap_topk(const float* centre_maps, const float* size_maps, float* candidates, int N, int H, int W, int k,
                     float image_size, void* stream);
int lhn_pck_accuracy(const float* pred, const float* gt, const uint8_t* mask /*[N,K]*/,
                     const float* normalize /*[N,2]*/, float thr, float* acc /*[K]*/,
                     float* avg_cnt /*[2]: avg, cnt*/, int N, int K, void* stream);
/* Streaming dataset-level evaluation: base_dataset.py:193-261 (_report_metric) = keypoint_pck_accuracy (top_down_eval.py:129-165),
 * keypoint_auc (:168-196) and keypoint_epe (:104-126) over the concatenated predictions of a test set, all three on
 * _calc_distances / _distance_acc (:12-62).  Every figure but EPE's numerator is a ratio of per-joint integer counts, so
 * the state is added to batch by batch (any split, any order, any number of devices) and divided once.
 * state: ONE device allocation of lhn_eval_state_bytes(K, num_step) bytes, zeroed by the caller before the first batch,
 * int64 words throughout (so states of several processes are merged by adding them word by word):
 *   [0,  K)              valid_pck[k]     samples of joint k with mask != 0 and no zero in their PCK normaliser
 *   [K,  2K)             hit_pck[k]       ... of those with distance < pck_thr
 *   [2K, 3K)             valid_auc[k]     samples of joint k with mask != 0 (and auc_normalize != 0)
 *   [3K, 3K+num_step*K)  hit_auc[i][k]    ... of those with distance < float32(i / num_step)
 *   then 4 words         epe_cnt          masked-in keypoints
 *                        epe_hi, epe_lo   sum of their float32 distances in exact fixed point: whole pixels, and the
 *                                         fractions in units of 2^-32 px (each rounded to that unit: <= 2^-33 px off)
 *                        epe_bad          distances that are inf, NaN or >= 2^62 px (EPE then reads NaN)
 * Integer atomics only: the state after a batch does not depend on workgroup order, with or without LHN_DETERMINISTIC.
 * Arithmetic follows the reference's three routes: PCK float32 / float32 normaliser, EPE float32 / ones, AUC float32
 * difference / integer normaliser = float64 up to the root, rounded to float32 once.
 * lhn_eval_state_bytes is host-only (no device needed); 0 = unsupported (K, num_step): (3 + num_step) * K <= 8192.
 * pck_normalize [N,2] may be NULL: the PCK counts are then left alone (keypoint_auc / keypoint_epe on their own).
 * lhn_eval_finalize: out = double[K + 4] = acc[K] (-1 for a joint without a valid sample) | pck (mean of acc >= 0) |
 * cnt (joints in that mean) | auc | epe, computed on the device. */
int64_t lhn_eval_state_bytes(int K, int num_step);
int lhn_eval_accumulate(const float* pred /*[N,K,2]*/, const float* gt /*[N,K,2]*/, const uint8_t* mask /*[N,K]*/,
                        const float* pck_normalize /*[N,2] or NULL*/, float pck_thr, double auc_normalize, int num_step,
                        void* state, int N, int K, void* stream);
int lhn_eval_finalize(const void* state, int K, int num_step, double* out /*[K+4]*/, void* stream);
/* acc: double[68]: [0..3] = {S_pos, S_neg, n_pos (exact integer < 2^53), unused} after the call,
 * [4..67] = 16 replicated partial-sum slots (spread the atomics); zeroed by the call */
int lhn_loss_balanced_mse_fwd(const float* out, const float* target, const float* weight /*[N,K]*/,
                              double* acc, float* loss /*[1]*/, int64_t NK, int64_t HW, float loss_weight,
                              int balance, void* stream);
int lhn_loss_balanced_mse_bwd(const float* out, const float* target, const float* weight,
                              const double* acc, const float* dloss /*[1] or NULL=1*/, float* dout,
                              int64_t NK, int64_t HW, float loss_weight, int balance, void* stream);

/* ---------------------------------------------------------------- conv building blocks (NHWC)
 * lhn_conv_pw_*    1x1 convolution of RepConv / nn.Conv2d            repblocks.py:8-44
 * lhn_conv_dw_*    depthwise k x k (dilation, stride) of RepConv     repblocks.py:8-44, liteHandNet.py:8-21
 * lhn_conv_stem_*  dense k x k on the 3-channel NCHW image           litehourglass.py:170, liteHandNet.py:175
 * lhn_conv_kxk_*   dense 3x3 (BasicBlock / BottleNeck)               liteHandNet.py:23-54
 * lhn_bn_finalize  train/eval BatchNorm2d statistics -> table        torch.nn.BatchNorm2d semantics
 * stats: double[LHN_STAT_REPLICAS][2][Cout] (sum, sum of squares), accumulated with atomics; caller zeroes.
 * weight gradients: `dw` may be replica 0 of `nrep` partial copies `rep_stride` floats apart (a block adds
 * into replica blockIdx % nrep; lhn_reduce_replicas folds them); nrep = 1 adds straight into dw.
 */
int lhn_conv_pw_fwd(const lhn_view* x, const float* w /*[Cout,Cin]*/, const float* bias /*or NULL*/,
                    const lhn_view* y, double* stats /*or NULL*/, int stride, float* y_nchw /*or NULL*/,
                    const lhn_bnfin* fin /*or NULL*/, void* stream);
/* Extended 1x1 entry points.  Any channel counts that are multiples of 4 (hourglassnet.py: 256; lite_hrnet.py: 20..320): the
 * library runs (<=128) x (<=128) channel slices itself (input slices accumulate into y; bias and BatchNorm statistics on the
 * last one).  opts (NULL = defaults):
 *   w_cols / w_rows   real shape of the weight tensor when the views are padded to a multiple of 4 (the 21-joint head of
 *                     hourglassnet.py:117 stored as 24 NHWC channels, and merge_preds :119 reading them back);
 *   nchw_batch_stride floats between two images of the NCHW tensor (the stacked [N, num_stack, K, H, W] output, :136). */
typedef struct lhn_pw_opts {
  int32_t w_cols, w_rows;
  int64_t nchw_batch_stride;
  /* forward only: the consumed input is coef[0]*value(x) + sum_e coef[e+1]*value(extra[e]) -- residual sums taken on load
   * (litehourglass.py:41-49) instead of being materialised by lhn_ew_fwd.  Same geometry and channel count as x. */
  int32_t n_extra;              /* 0..2 */
  const lhn_view* extra;
  float coef[3];
  /* with extra sources: the summed input is ALSO written here (plain values; same pixels and channel count as x).  A
   * training forward leaves the sum where the backward's weight gradient reads it -- one write instead of a separate
   * elementwise pass that re-reads every operand.  NULL: not written. */
  const lhn_view* sum_out;
} lhn_pw_opts;
int lhn_conv_pw_fwd2(const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats, int stride,
                     float* y_nchw, const lhn_bnfin* fin, const lhn_pw_opts* opts, void* stream);
int lhn_conv_dw_fwd(const lhn_view* x, const float* w /*[C,1,k,k]*/, const lhn_view* y, double* stats,
                    int k, int stride, int pad, int dil, const lhn_bnfin* fin, void* stream);
/* depthwise 3x3 (stride 1, 'same' padding, dilation 1/2) over coef2[0]*value(x) + coef2[1]*value(extra): MSRB's second
 * round reads `out + ca(cat)` (litehourglass.py:41-45) without an elementwise pass in between.  extra == NULL: lhn_conv_dw_fwd. */
int lhn_conv_dw_fwd2(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int k, int stride, int pad, int dil,
                     const lhn_bnfin* fin, const lhn_view* extra, const float* coef2 /*host, 2 floats*/, void* stream);
/* ... and sum_out (or NULL): the summed input is also written there, see lhn_pw_opts.sum_out. */
int lhn_conv_dw_fwd3(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int k, int stride, int pad, int dil,
                     const lhn_bnfin* fin, const lhn_view* extra, const float* coef2, const lhn_view* sum_out, void* stream);
/* Inference only: RepBasicUnit's right branch, RepConv 1x1 then RepConv depthwise 3x3 (litehourglass.py:52-78 over
 * repblocks.py:8-44), in one launch -- the tensor between the two convolutions never reaches memory.  Per image:
 *   t     = lrelu_slope1(scale1 * (w1 . value(x)) + shift1)      t_table = [3][Cm] scale | shift | slope (NULL = identity)
 *   y_raw = depthwise 3x3 of t, stride 1, dilation 1, t padded with ZEROS (not with lrelu(shift1))
 * y_raw is stored raw into channels [y.coff, y.coff + Cm) of y; its own bias / BatchNorm / activation stay pending in y's
 * table exactly as lhn_conv_dw_fwd leaves them.  No statistics, no atomics: repeated calls give identical bits.
 * Built for Cin == Cm == 64 (any N, H, W); any other channel count returns the invalid-argument status and writes nothing. */
int lhn_conv_pw_dw3_fwd(const lhn_view* x, const float* w1 /*[Cm,Cin]*/, const float* t_table /*[3][Cm] or NULL*/,
                        const float* w2 /*[Cm,1,3,3]*/, const lhn_view* y, void* stream);
/* Inference only: DWConv (liteHandNet.py:8-21 over repblocks.py:8-44), RepConv depthwise 3x3 then RepConv 1x1, in one launch --
 * the tensor between the two convolutions never reaches memory.  Per image:
 *   u     = depthwise 3x3 of value(x), stride 1, dilation dil (1 or 2), padding dil; value(x) padded with ZEROS
 *   t     = lrelu_slope(scale * u + shift)            t_table = [3][Cin] scale | shift | slope (NULL = identity)
 *   y_raw = w_pw . t (+ bias)                          stored raw into channels [y.coff, y.coff + Cout) of y
 * value(x) is the view's own table and gate applied on load, exactly as lhn_conv_dw_fwd3 does; a pixel outside the map is 0, not
 * lrelu(shift_x).  y keeps its own pending BatchNorm / activation in its table as lhn_conv_pw_fwd leaves them.  No statistics, no
 * atomics: repeated calls give identical bits.  Built for Cin, Cout in {32, 64} (any N, H, W); any other channel count, a dilation
 * outside {1, 2} or a y view that overlaps x's channels in the same buffer returns the invalid-argument status ("unsupported
 * shape") and writes nothing. */
int lhn_conv_dw3_pw_fwd(const lhn_view* x, const float* w_dw /*[Cin,1,3,3]*/, int dil, const float* t_table /*[3][Cin] or NULL*/,
                        const float* w_pw /*[Cout,Cin]*/, const float* bias /*[Cout] or NULL*/, const lhn_view* y, void* stream);
/* Inference only: BottleNeck (liteHandNet.py:23-37 over repblocks.py:8-44) in one launch -- the three intermediate tensors never
 * reach memory.  Per image:
 *   t1 = act1(w1 . value(x) (+ b1))      1x1, C -> Cm          act_i(v) = t_i ? lrelu_{slope_i}(scale_i*v + shift_i) : v
 *   t2 = act2(conv3x3(t1))               Cm -> Cm, stride 1, t1 padded with ZEROS (not with act1(shift))
 *   t3 = act3(w3 . t2 (+ b3))            1x1, Cm -> C
 *   y  = lrelu_{out_slope}(value(x) + t3)   stored PLAIN into channels [y.coff, y.coff + C) of y, as lhn_ew_fwd leaves it
 * value(x) is the view's own table and gate applied on load, as lhn_conv_dw3_pw_fwd does.  t1, t2 = [3][Cm], t3 = [3][C] scale | shift |
 * slope tables (NULL = identity); Cm is the middle channel count (the weights carry no shape).  All three convolutions run on the
 * fp32 MFMA; no statistics, no atomics: repeated calls give identical bits, with or without LHN_DETERMINISTIC.
 * wt_scratch: optional 9*Cm*Cm floats of caller-owned scratch; the call re-lays w2 tap-major into it with one small launch of its own
 * (16-byte weight loads per tap), as lhn_conv_kxk_fwd does.  NULL = the kernel reads the OIHW tensor directly and the call is ONE
 * launch.  (The plan executor skips the re-lay when the parameters have not changed since the run that wrote the scratch.)
 * Built for C == 128 with Cm in {32, 64} and C == 256 with Cm in {64, 128}, any N, H, W.  Any other channel pair, an out_slope outside [0, 1] (LHN_SLOPE_SILU /
 * LHN_SLOPE_RELU_SIGMOID) or a y view that overlaps x's channels in the same buffer returns the invalid-argument status
 * ("unsupported shape") before any launch and writes nothing. */
int lhn_bottleneck_fwd(const lhn_view* x, int Cm, const float* w1 /*[Cm,C]*/, const float* b1 /*[Cm] or NULL*/, const float* t1 /*[3][Cm] or NULL*/,
                       const float* w2 /*[Cm,Cm,3,3]*/, const float* t2 /*[3][Cm] or NULL*/,
                       const float* w3 /*[C,Cm]*/, const float* b3 /*[C] or NULL*/, const float* t3 /*[3][C] or NULL*/,
                       float out_slope, const lhn_view* y, float* wt_scratch /*9*Cm*Cm floats or NULL*/, void* stream);
/* Inference only: the stem after its first convolution (Stem.forward, liteHandNet.py:169-193; my_pelee_stem,
 * models/pose_hg_ms_att.py:196-228) in one launch -- the depthwise K x K, branch1 (1x1, dense 3x3 stride 2), branch2 (max pool), the
 * concatenation and the last 1x1; no intermediate tensor reaches memory.  Per image, with m = x.C = 32 and C = y.C = 128:
 *   t = K ? actT(dwKxK(value(x)) (+ bT)) : value(x)     K in {0, 3, 7}; stride 1, pad K/2; x outside the map is 0, not act(shift_x)
 *   u = actU(w1 . t (+ b1))                              1x1, m -> m, at H x W
 *   v = actV(conv3x3(u) (+ b2))                          dense, m -> m, stride 2, pad 1; u padded with ZEROS (not with actU(shift))
 *   p = maxpool2x2(t), stride 2, ceil_mode               windows clipped to the map; tables are applied BEFORE the max
 *   y = w3 . cat(v, p) (+ b3)                            1x1, 2m -> C, at ceil(H/2) x ceil(W/2); stored raw into channels
 *                                                        [y.coff, y.coff + C) of y, as lhn_conv_pw_fwd leaves it
 * actX(v) = tX ? lrelu_{slope}(scale*v + shift) : v with tT, tU, tV = [3][m] scale | shift | slope tables (NULL = identity); biases may
 * be NULL; value(x) is the view's own table and gate applied on load.  K = 0: x IS t (the eval-mode RepBlock sum, stored plain by
 * lhn_ew_fwd) and w_dw, bT, tT are ignored.  All three dense stages run on the fp32 MFMA with fp32 accumulation; no statistics, no
 * atomics: repeated calls give identical bits, with or without LHN_DETERMINISTIC.
 * wt_scratch: optional 9*m*m floats of caller-owned scratch; the call re-lays w2 tap-major into it with one small launch of its own, as
 * lhn_bottleneck_fwd does.  NULL = the kernel reads the OIHW tensor directly (the same products in the same order: the same bits) and
 * the call is ONE launch.  (The plan executor skips the re-lay when the parameters have not changed since the run that wrote it.)
 * Built for m == 32, C == 128, K in {0, 3, 7}, any N, H, W >= 1 (H, W may be odd; y is N x ceil(H/2) x ceil(W/2)).  Any other channel
 * pair, any other K, a table slope outside [0, 1] (LHN_SLOPE_SILU / LHN_SLOPE_RELU_SIGMOID; x's own table included -- this entry point
 * waits for the stream and reads the slope rows back, so it cannot be called on a capturing stream) or a y view that overlaps x's
 * channels in the same buffer returns the invalid-argument status ("unsupported shape") before any launch and writes neither y nor
 * the scratch. */
int lhn_stem_tail_fwd(const lhn_view* x, int K, const float* w_dw /*[m,1,K,K]; unused when K == 0*/, const float* bT /*[m] or NULL*/,
                      const float* tT /*[3][m] or NULL*/, const float* w1 /*[m,m]*/, const float* b1 /*[m] or NULL*/,
                      const float* tU /*[3][m] or NULL*/, const float* w2 /*[m,m,3,3]*/, const float* b2 /*[m] or NULL*/,
                      const float* tV /*[3][m] or NULL*/, const float* w3 /*[C,2m]*/, const float* b3 /*[C] or NULL*/, const lhn_view* y,
                      float* wt_scratch /*9*m*m floats or NULL*/, void* stream);
/* Inference only: one round of an MSRB (litehourglass.py:13-50 over repblocks.py:8-44, common.py:23-66) as one pass over the
 * feature map -- both dilated depthwise 3x3 branches in one launch and, with pooled != NULL, the adaptive-average-pool means the
 * round's ChannelAttension (OH = OW = 3) or SEBlock (OH = OW = 1) reads.  Half k (k = 0: dilation 1, padding 1; k = 1: dilation 2,
 * padding 2; stride 1) consumes  coef2[0] * value(x[k]) + coef2[1] * value(extra[k])  (extra == NULL: value(x[k]) alone), the
 * form lhn_conv_dw_fwd2 accepts; x[0], x[1] (and extra[0], extra[1]) are separate views of C/2 channels each, with their own
 * buffer, cstride, coff, table and gate.  value() is the view's table and gate applied on load as lhn_conv_dw_fwd3 does; a pixel
 * outside the map is 0, not lrelu(shift).  The raw results go to channels [y.coff, y.coff + C/2) and [y.coff + C/2, y.coff + C)
 * of y; the BatchNorm / bias of each branch stays pending in y's table as lhn_conv_dw_fwd leaves it.
 *   pooled[n, oh, ow, c] = mean over rows [floor(oh*H/OH), ceil((oh+1)*H/OH)) and the columns likewise of y's CONSUMED value: y's
 *   table (current before the call; y has no gate yet) applied to the raw result -- what lhn_avgpool_fwd(y, pooled, OH, OW) would
 *   write after the two depthwise launches, up to fp32 summation order.
 * No float atomics: the launch writes per-(tile, bin, channel) sums into `scratch` (lhn_msrb_round_scratch_bytes, caller-owned, no
 * initialisation needed) and a small second kernel of the same call folds them in a fixed order; repeated calls give identical
 * bits.  Built for C/2 in {32, 64, 128}, any N, H, W.  Any other channel count, OH != OW or OH outside {1, 3} with pooled, pooled
 * without scratch, or a y view that overlaps x[k] / extra[k] in the same buffer returns the invalid-argument status ("unsupported
 * shape") and writes nothing. */
int64_t lhn_msrb_round_scratch_bytes(int N, int H, int W, int C);   /* host-only, like lhn_eval_state_bytes; 0 = unsupported */
int lhn_msrb_round_fwd(const lhn_view x[2], const lhn_view* extra /*[2] or NULL*/, const float* coef2 /*host, 2 floats, or NULL*/,
                       const float* w_d1 /*[C/2,1,3,3]*/, const float* w_d2 /*[C/2,1,3,3]*/, const lhn_view* y /*C channels*/,
                       float* pooled /*[N,OH,OW,C] or NULL*/, int OH, int OW, void* scratch, void* stream);
/* Cout = 8, 16, .. 256 (a power of two times 8) or 40 (the stem of mynet at input_channel = 160), k = 1, 3, 5 or 7.  3x3 -> 32 and
 * 7x7 -> 64 run on MFMA kernels; every other shape on the direct kernel, which keeps the weights and its reduction scratch in 3*k*k*Cout*4 + 16384 bytes of LDS: a shape that
 * needs more than 65536 bytes (k = 7 with Cout >= 128, k = 5 with Cout = 256) returns the invalid-argument status before any
 * launch, with the byte count in the text, and writes nothing. */
int lhn_conv_stem_fwd(const float* img /*[N,3,Hi,Wi]*/, const float* w /*[Cout,3,k,k]*/, const lhn_view* y,
                      double* stats, int Hi, int Wi, int k, int stride, int pad, const lhn_bnfin* fin, void* stream);
/* wt_scratch: optional 9*Cout*Cin floats of caller-owned scratch; the call re-lays the OIHW weights tap-major into it
 * (16-byte weight loads per tap instead of 36-byte-strided gathers).  NULL = read the OIHW tensor directly.
 * Cin in {32, 64, 128, 256}; Cout in {32, 64, 128, 256} (1, 2, 4 or 8 tiles of 32 features; a Cout whose tile count is one of
 * these may end in a partial tile, e.g. 40).  Cin = 256 runs as two 128-channel K slices per tap inside one launch, Cout = 256 as
 * blocks of at most 128 features on gridDim.y; statistics and the fused finalize (`fin`) see the complete sums either way.
 * Width 160 (mynet's own convolutions, and no other pair with one of these sides): 160 -> 160 runs as five 32-channel K slices per tap
 * with the five feature tiles in one block or one per block on gridDim.y = 5; 40 -> 40 runs on the 64-channel LDS images with
 * channels [40, 64) zero (their lanes issue no x load; the MFMA loop stops after channel 39).  Five feature tiles exist for
 * 160 alone: a Cout or Cin of 129 .. 159 is refused.  Any
 * other channel count returns the invalid-argument status ("unsupported channels") before the first launch and writes nothing,
 * the scratch included.  wt_scratch holds 9*Cout*Cin floats ([tap][Cout][Cin]; 589,824 floats = 2.25 MiB at 256 -> 256). */
int lhn_conv_kxk_fwd(const lhn_view* x, const float* w /*[Cout,Cin,3,3]*/, const lhn_view* y, double* stats,
                     int stride, const lhn_bnfin* fin, float* wt_scratch, void* stream);
/* Inference only: the stride-1 dense 3x3 of lhn_conv_kxk_fwd (liteHandNet.py:31,45: RepConv(.., 3, 1, 1) of BottleNeck / BasicBlock;
 * hourglassnet.py:33 Residual.conv2; nn.Conv2d(Cin, Cout, 3, 1, 1) on fp32) on the bf16 MFMA with a three-term split ("bf16x3"): every fp32 operand is
 * hi + lo with hi = bf16(v), lo = bf16(v - hi) (round-to-nearest-even) and  a*b ~ a_lo*b_hi + a_hi*b_lo + a_hi*b_hi  with fp32
 * accumulation, added in that order per 16 input channels, taps 0..8, channels ascending.  Per element the result stays within
 * 3.1 * 2^-16 * conv(|value(x)|, |w|) of the exact convolution (about 17 x the error of the fp32 kernel on activations).
 * value(x) is the view's table, slope and gate applied in fp32 on load, as lhn_conv_kxk_fwd does; the map is padded with zeros of
 * the VALUE.  y gets the raw sums in channels [y.coff, y.coff + Cout); no statistics, no bias, no atomics: repeated calls give
 * identical bits, with or without LHN_DETERMINISTIC.
 * wsplit: caller-owned scratch of 9*Cout*Cin*4 bytes (the size of lhn_conv_kxk_fwd's wt_scratch), REQUIRED.  relay = 1: the call first
 * writes the split tap-major image of w into it ([2][9][Cout][Cin] bf16: hi, then lo) with one small launch; relay = 0: it already
 * holds the image of these weights (the plan executor, when the parameters have not changed since the run that wrote it).
 * Built for Cin, Cout in {32, 64, 128}, any N, H, W, channel-slice views.  A y map that is not x's (stride != 1), any other channel
 * count, wsplit == NULL or a y view that overlaps x's channels in the same buffer returns the invalid-argument status before any
 * launch and writes nothing. */
int lhn_conv_kxk_fwd_bf16x3(const lhn_view* x, const float* w /*[Cout,Cin,3,3]*/, const lhn_view* y,
                            void* wsplit /* 9*Cout*Cin*4 bytes, required */, int relay /* 1: rebuild wsplit from w */, void* stream);
/* conv_bias: a biased convolution followed by BatchNorm (models/pose_hg_ms_att.py:27-35,46-56) stores its output
 * WITHOUT the bias -- BatchNorm cancels it -- and the bias only enters the running mean (training) or the shift
 * (eval: beta - (running_mean - bias) * scale).  d(bias) is identically zero in training mode.
 * training = 0: the table comes from the running statistics; running_mean, running_var, num_batches_tracked and
 * save_mean_invstd are not written (there are no batch statistics to save). */
int lhn_bn_finalize(const double* stats, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, int64_t* num_batches_tracked, float* table, int cstride, int coff,
                    int C, float* save_mean_invstd /*[2][C]*/, double count, float eps, float momentum,
                    float slope, int training, const float* conv_bias /*or NULL*/, void* stream);
/* stat_channels >= C: the statistics / save arrays were laid out for a view padded to a multiple of 4 (lite_hrnet.py:84-96:
 * BatchNorm over 7 / 17 / 37 channels behind a 1x1 whose output view has 8 / 20 / 40) */
int lhn_bn_finalize2(const double* stats, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, float* table, int cstride, int coff, int C, int stat_channels,
                     float* save_mean_invstd, double count, float eps, float momentum, float slope, int training,
                     const float* conv_bias, void* stream);
int lhn_table_fill(float* table, int cstride, int coff, int C, float scale, float shift, float slope,
                   void* stream);

/* elementwise / pooling (liteHandNet.py:88-113, litehourglass.py:136-163, common.py:40-66) */
/* pending transform of a deployed (biased, BN-free) convolution: table slice = (1, bias[c] or 0, slope)
 * -- RepConv.forward with rep_conv, repblocks.py:41-43 */
int lhn_table_bias(float* table, int cstride, int coff, int C, const float* bias /*or NULL*/, float slope,
                   void* stream);
/* deploy-time re-parameterisation (repblocks.py:46-73,169-236; common.py:68-90): one branch of the fused kernel.
 * out_w[Cout][cin_g][k][k] (store | +=) branch * gamma/sqrt(rvar+eps), branch = w (kb x kb centred in k x k) or the
 * identity kernel when w == NULL; out_b[Cout] (store | +=) beta - rmean*gamma/sqrt(rvar+eps).  Equals the IEEE float32
 * evaluation of the reference's formula bit for bit when the branches are added in the order 1x1, identity, k x k. */
int lhn_fold_bn(const float* w, int kb, const float* gamma, const float* beta, const float* rmean,
                const float* rvar, float eps, float* out_w, float* out_b, int Cout, int cin_g, int k,
                int accumulate, void* stream);
/* out_slope == LHN_SLOPE_SILU selects SiLU instead of a leaky ReLU as the combine's output activation (the
 * BN -> SiLU -> conv pre-activation unit of models/pose_hg_ms_att.py:76-90; single same-size source in backward) */
#define LHN_SLOPE_SILU 2.0f
/* out_slope == LHN_SLOPE_RELU_SIGMOID: sigmoid(relu(v)) -- the nn.ReLU + nn.Sigmoid pairs of lite_hrnet.py:62-70,86-97
 * (single same-size source in backward, like SiLU) */
#define LHN_SLOPE_RELU_SIGMOID 3.0f
int lhn_ew_fwd(const lhn_view* srcs, int nsrc, const lhn_view* dst, float out_slope, void* stream);
/* dst = act(sum_i coef[i] * value_i); coef == NULL: all ones (host pointer, nsrc floats) */
int lhn_ew_fwd2(const lhn_view* srcs, int nsrc, const float* coef, const lhn_view* dst, float out_slope, void* stream);
/* mode bit 0: PRODUCT of the sources instead of their sum (lite_hrnet.py:105-107, s * F.interpolate(a, nearest));
 * mode bit 1: smaller sources are resampled bilinearly with align_corners=True (lite_hrnet.py:272-275) instead of nearest.
 * Backward of the product: lhn_ew_mul_bwd per operand; of a bilinear source: lhn_bilinear_bwd (same-size sources of
 * that combine: lhn_ew_bwd2 as usual). */
int lhn_ew_fwd3(const lhn_view* srcs, int nsrc, const float* coef, const lhn_view* dst, float out_slope, int mode, void* stream);
int lhn_ew_mul_bwd(const lhn_view* src, const lhn_view* other, const lhn_view* dst, const float* ddst, float* dsrc,
                   int accumulate, void* stream);
/* out_slope: a leaky slope (its derivative is read from the stored dst); LHN_SLOPE_SILU / LHN_SLOPE_RELU_SIGMOID are refused */
int lhn_bilinear_bwd(const lhn_view* src, const lhn_view* dst, const float* ddst, float* dsrc, int accumulate, float out_slope,
                     void* stream);
/* channel_shuffle(torch.cat([a, b], 1), groups = 2) (lite_hrnet.py:29-52,141-142,246-247): dst[2j] = value(a)[j],
 * dst[2j+1] = value(b)[j]; dst stored plain.  Backward hands d(dst) back to the operands' gradient buffers. */
int lhn_shuffle2_fwd(const lhn_view* a, const lhn_view* b, const lhn_view* dst, void* stream);
int lhn_shuffle2_bwd(const lhn_view* a, const lhn_view* b, const lhn_view* dst, const float* ddst, float* da, int acc_a,
                     float* db, int acc_b, void* stream);
/* ConditionalChannelWeighting (lite_hrnet.py:110-143) of an inference plan as four grouped launches: every call serves all B = 2..4
 * branches of the block in ONE grid.  Branch b has x2[b] (the upper half of the block's input, [N, H_b, W_b, C_b]), x1[b] (the lower
 * half), y[b] (the depthwise convolution's raw output; its table is the eval-mode BatchNorm with the convolution's bias folded in)
 * and out[b] (2 * C_b channels).  The smallest map (hm, wm) is the last branch's, Ct = sum of C_b; tables and gates of the inputs
 * are applied on load.
 *   lhn_ccw_pool_fwd     pooled[N, hm, wm, Ct]: branch b's channels at their running offset = adaptive_avg_pool2d(value(x2[b]), (hm, wm))
 *   lhn_ccw_gate_fwd     g[npix, Ct] = sigmoid(relu(t2(W2 . sigmoid(relu(t1(W1 . pooled)))))) per pooled pixel; t1 / t2: [3][t*_stride]
 *                        eval tables (bias folded into the shift, as lhn_bn_finalize with conv_bias does) of which the first mid / Ct
 *                        columns are read; Ct <= 320, mid <= 40, any values inside
 *   lhn_ccw_dw_fwd       y[b] = dw3x3(value(x2[b]) * up(g_b)), stride 1, zero padding of the PRODUCT, up = nearest upsample by
 *                        H_b / hm; every tile also writes the per-channel sum of value(y[b]) over its pixels into `scratch`
 *   lhn_ccw_shuffle_fwd  per workgroup: folds its sample's tile sums in a fixed order to the global mean, runs the SpatialWeighting
 *                        MLP (C_b -> J -> C_b, the arithmetic of lhn_se_mlp_fwd2 mode 1), then stores out[b][2j] = value(x1[b])[j],
 *                        out[b][2j+1] = value(y[b])[j] * gate[n][j], plain like lhn_shuffle2_fwd.  y[b].gate is not read: the gate
 *                        lives in the launch.
 * No float atomics: repeated calls give identical bits.  B outside 2..4, a map that is not an integer multiple of the last one,
 * branches not ordered from the largest map to the smallest, C_b above 160 (or J outside 1..40), an output that overlaps an input's
 * channels in the same buffer or a missing scratch returns the invalid-argument status ("unsupported shape") before any launch and
 * writes nothing.  Any N, any map size down to 1 x 1. */
typedef struct lhn_ccw_se {
  const float *w1 /*[J,C]*/, *b1 /*[J] or NULL*/, *w2 /*[C,J]*/, *b2 /*[C] or NULL*/;
  int32_t J;
} lhn_ccw_se;
int64_t lhn_ccw_scratch_bytes(int N, int B, const int* H, const int* W, const int* C);   /* host-only; 0 = unsupported */
int lhn_ccw_pool_fwd(const lhn_view* x2 /*[B]*/, int B, float* pooled, void* stream);
int lhn_ccw_gate_fwd(const float* pooled, int64_t npix, int Ct, int mid, const float* w1 /*[mid,Ct]*/, const float* t1, int t1_stride,
                     const float* w2 /*[Ct,mid]*/, const float* t2, int t2_stride, float* g, void* stream);
int lhn_ccw_dw_fwd(const lhn_view* x2 /*[B]*/, int B, const float* g /*[N,hm,wm,Ct]*/, const float* const* w /*[B] of [C_b,1,3,3]*/,
                   const lhn_view* y /*[B]*/, void* scratch, void* stream);
int lhn_ccw_shuffle_fwd(const lhn_view* x1 /*[B]*/, const lhn_view* y /*[B]*/, int B, const lhn_ccw_se* se /*[B]*/, const void* scratch,
                        const lhn_view* out /*[B]*/, void* stream);
int lhn_maxpool2_fwd(const lhn_view* x, const lhn_view* y, void* stream);
int lhn_avgpool_fwd(const lhn_view* x, float* out /*[N,OH,OW,x.C]*/, int OH, int OW, void* stream);
/* ... into channels [out_coff, out_coff + x.C) of an [N,OH,OW,out_cstride] tensor: the pooled branches of
 * CrossResolutionWeighting land side by side, torch.cat needs no copy (lite_hrnet.py:99-102) */
int lhn_avgpool_fwd2(const lhn_view* x, float* out, int OH, int OW, int out_cstride, int out_coff, void* stream);
int lhn_avgpool_bwd2(const lhn_view* x, const float* dout, int OH, int OW, int out_cstride, int out_coff, float* dx,
                     int dx_accumulate, void* stream);
/* gamma == NULL: deployed attention, `beta` is the bias of the fused depthwise conv, no BatchNorm (eval only) */
int lhn_ca_mlp_fwd(const float* pooled /*[N,9,C]*/, const float* w3 /*[C,1,3,3]*/, const float* gamma,
                   const float* beta, float* rmean, float* rvar, int64_t* nbt, const float* w1 /*[C/2,C]*/,
                   const float* b1, const float* w2 /*[C,C/2]*/, const float* b2, const float* dropmask,
                   float* gate, int gate_stride, int gate_coff, float* save /*see DESIGN*/, int N, int C,
                   float eps, float momentum, int training, int stage, double* gsum, double count_scale,
                   void* stream);
/* SyncBatchNorm (train/spawn_dist.py:37-38) support in the attention kernels: stage 0 = the whole op; stage 1 = up to
 * the local statistics sums, written to gsum[2][C] for the caller to all-reduce; stage 2 = the rest, with statistics
 * over N*count_scale samples.  Backward: pgrad_scale (1/world) scales d(gamma), d(beta), which come from global sums. */

/* attention of `mynet` (models/pose_hg_ms_att.py:165-174,191-192) on the pooled [N,9,C] tensor:
 * gate = sigmoid(Linear(dropout(dw3x3(relu(BN(pooled))) + b3))); save = floats[3*N*C + 2*C]
 * refused: N <= 0, C outside 1..256, gate_stride < gate_coff + C (backward: cstride < coff + C), a stage outside 0..2, stage 1 / 2
 * without gsum or with count_scale < 1.
 * backward: H < 2 or W < 2 is refused -- the segment layout of the pooled gradient (one slot per pixel) needs two pixels per axis */
int lhn_att_mlp_fwd(const float* pooled, const float* gamma, const float* beta, float* rmean, float* rvar,
                    int64_t* nbt, const float* w3 /*[C,1,3,3]*/, const float* b3, const float* wl /*[C,C]*/,
                    const float* bl, const float* dropmask /*[N,C] or NULL*/, float* gate, int gate_stride,
                    int gate_coff, float* save, int N, int C, float eps, float momentum, int training, int stage,
                    double* gsum, double count_scale, void* stream);
int lhn_att_mlp_bwd(const float* pooled, const float* gamma, const float* beta, const float* w3, const float* wl,
                    const float* dropmask, float* save, const float* dgate /*[N,C]*/, float* dpool, int cstride,
                    int coff, int H, int W, float* dgamma, float* dbeta, float* dw3, float* db3, float* dwl,
                    float* dbl, int N, int C, int stage, double* gsum, double count_scale, float pgrad_scale,
                    void* stream);

/* squeeze-and-excitation gate (models/pose_estimation/liteHandNet/common.py:23-37; ca_type / msrb_ca / rbu_ca = 'se'):
 * gate = sigmoid(up(relu(down(pooled)))), pooled = lhn_avgpool_fwd(y, 1, 1) [N,C]; J = internal neurons; save = floats[N*J + N*C] */
int lhn_se_mlp_fwd(const float* pooled, const float* w1 /*[J,C]*/, const float* b1, const float* w2 /*[C,J]*/,
                   const float* b2, float* gate, int gate_stride, int gate_coff, float* save, int N, int C, int J,
                   void* stream);
/* mode 1: SpatialWeighting of lite_hrnet.py:55-74 -- sigmoid(relu(.)) after both 1x1 convolutions (mode 0 = SEBlock).
 * b1 and b2 (and db1, db2) may both be NULL: the bias-free nn.Linear pair of hourglass_ablation.py:201-209
 * refused: a mode other than 0 or 1; gate_stride < gate_coff + C (backward: cstride < coff + C); N <= 0, C outside 1..256, J outside 1..64 */
int lhn_se_mlp_fwd2(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                    int gate_stride, int gate_coff, float* save, int N, int C, int J, int mode, void* stream);
int lhn_se_mlp_bwd2(const float* pooled, const float* w1, const float* w2, const float* save, const float* dgate,
                    float* dpool, int cstride, int coff, int H, int W, float* dw1, float* db1, float* dw2, float* db2, int N,
                    int C, int J, int mode, void* stream);
int lhn_se_mlp_bwd(const float* pooled, const float* w1, const float* w2, const float* save, const float* dgate /*[N,C]*/,
                   float* dpool /*[N,25,cstride]*/, int cstride, int coff, int H, int W, float* dw1, float* db1, float* dw2,
                   float* db2, int N, int C, int J, void* stream);

/* backward building blocks */
int lhn_bn_bwd_reduce(const lhn_view* y, const lhn_gradview* g, const float* save_mean_invstd,
                      double* sums /*[R][2][C]: sum du, sum du*xhat*/, const lhn_bnbwdfin* fin /*or NULL*/, void* stream);
int lhn_bn_bwd_finalize(const double* sums, const float* gamma, const float* save_mean_invstd,
                        float* coef, int cstride, int coff, int C, double count, float* dgamma, float* dbeta,
                        float pgrad_scale /*1, or 1/world under SyncBatchNorm*/, void* stream);
int lhn_bn_bwd_finalize2(const double* sums, const float* gamma, const float* save_mean_invstd, float* coef, int cstride,
                         int coff, int C, int stat_channels, double count, float* dgamma, float* dbeta, float pgrad_scale,
                         void* stream);
int lhn_conv_pw_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy,
                    float* dx /*grad buffer of x, same geometry, or NULL*/, int dx_accumulate, float* dw,
                    float* dbias, int stride, const float* dy_nchw, int nrep, int64_t rep_stride, void* stream);
int lhn_conv_pw_bwd2(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                     int dx_accumulate, float* dw, float* dbias, int stride, const float* dy_nchw, int nrep, int64_t rep_stride,
                     const lhn_pw_opts* opts, void* stream);
int lhn_conv_dw_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                    int dx_accumulate, float* dw, int k, int stride, int pad, int dil, int nrep, int64_t rep_stride,
                    void* stream);
/* ... and, when this convolution is the only reader of x and x is the output of a convolution + BatchNorm, the
 * BatchNorm-backward sums of THAT producer (sum du, sum du * xhat into bn_sums[LHN_STAT_REPLICAS][2][bn_C] at channel
 * bn_coff, mean / invstd from bn_save) -- the kernel has d(x), the raw x and its table in hand; lhn_bn_bwd_reduce of the
 * producer is then skipped.  3x3, stride 1, dilation 1, dx stored (not accumulated), x ungated.  bn_sums NULL: no sums. */
int lhn_conv_dw_bwd2(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, int k, int stride, int pad, int dil, int nrep, int64_t rep_stride, double* bn_sums,
                     const float* bn_save, int bn_C, int bn_coff, void* stream);
/* ... and with up to two gradient ADDENDS: dx = [dx +] dgrad + dx_add0 + dx_add1, where dx_add* point at buffers of dx's
 * geometry (same pixel stride; the pointer already carries any channel shift).  They are the output gradients of residual
 * sums that read x (litehourglass.py:41-49: `out = out + ca(cat)`): the sum's backward costs no pass of its own.  Needs the
 * tiled kernel (stride 1, "same" padding, W >= 8).  Both NULL: no addends. */
int lhn_conv_dw_bwd3(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, int k, int stride, int pad, int dil, int nrep, int64_t rep_stride, const float* dx_add0,
                     const float* dx_add1, void* stream);
/* Cout: a power of two times 4 up to 256, or 40; k = 1, 3 or 7 (anything else: the invalid-argument status, nothing written). */
int lhn_conv_stem_bwd(const float* img, const lhn_view* y, const lhn_gradview* gy, float* dw, int Hi, int Wi,
                      int k, int stride, int pad, int nrep, int64_t rep_stride, void* stream);
/* NOTE: lhn_conv_kxk_bwd and the large-channel path of lhn_conv_pw_bwd CONSUME gy->dz (it is overwritten in place
 * with dy before the MFMA kernels stream it).
 * lhn_conv_kxk_bwd: Cin, Cout in {32, 64, 128, 256} (3x3, pad 1, stride 1 or 2); anything else returns the invalid-argument status
 * ("unsupported channels") before the first launch: dz, dx, dw and the scratch are left as they were.  256 channels run as two
 * 128-channel slices: Cout = 256 inside the data-gradient kernel (dx is written once), Cin = 256 as one weight-gradient launch per
 * input slice.  160 -> 160 and 40 -> 40 as in lhn_conv_kxk_fwd (and 64 -> 40 without dx, as before): 160 is always plain, its data
 * gradient runs five 32-channel slices of Cout, its weight gradient a 128-channel and a 32-channel input slice with Cout on five or
 * three groups; 40 -> 40 is below the size rule, so dy is formed on the fly unless LHN_PLAIN=1 or a pooled gradient says otherwise.
 * wt_scratch: 9*Cout*Cin floats (589,824 at 256 -> 256), written [tap][Cin][Cout] by the call when dx != NULL, or NULL.
 * dz is consumed ("plain": k_dy_inplace in front) with a pooled gradient, with a side above 128, and otherwise when Cin * Cout >= 4096.
 * LHN_PLAIN=0 / 1 replaces that last size rule alone (never / always; it does not apply to a pooled gradient or a side above 128).  The
 * variable is read once, at the first dense 3x3 call or query of the process: set it before the process starts.
 * Which kernels a call launches is kxk_fwd_route / kxk_bwd_route's decision (csrc/k_conv_kxk.hip); lhn_conv_kxk_route below asks them. */
int lhn_conv_kxk_bwd(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx,
                     int dx_accumulate, float* dw, int stride, int nrep, int64_t rep_stride,
                     float* wt_scratch /*9*Cout*Cin floats or NULL, as above (dgrad layout)*/, void* stream);
/* Which kernels lhn_conv_kxk_fwd (backward = 0) / lhn_conv_kxk_bwd (backward = 1) launch for this shape, in order: host-only (no device
 * needed, nothing is launched), answered by the two functions the calls themselves ask.  N, H, W are x's; nrep as passed to the
 * backward call.  features: what the call carries.  cus: the compute units grids are sized for, <= 0 = what the library uses (the
 * device's; 2 under LHN_DETERMINISTIC=1; 256 without a device).  switches: -1 = as this process read LHN_PLAIN, else 0 or one of
 * LHN_KXK_SW_*.  Returns a static string (per thread, valid until the next call): the launches as a kernel trace prints them, joined
 * with " + ", each followed by the decisions its template arguments do not show --
 *   " yN"    N blocks of features on gridDim.y (forward: Cout, data gradient: Cin), where N > 1
 *   " par"   stride-2 data gradient: the four pixel-parity classes on gridDim.z
 *   " zN"    weight gradient: N groups of output channels on gridDim.z ("cosplit"), where N > 1
 *   " excl" / " atomic"   weight gradient: every block owns its slice of a gradient replica (read-add-write flush), or atomics
 *   " x 2"   weight gradient: one launch per 128-channel input slice (Cin = 256); Cin = 160 names its two launches, <128, ..> and <32, ..>
 * e.g. "k_dy_inplace + k_w_tapmajor + k_kxk<128, 1, 1, 9, true> y4 + k_kxk_wgrad<128, 1, 9, true> z4 excl"; profiles/kxk_instances.md and
 * profiles/kxk160_instances.md are printed from it.  NULL: no kernel instance (the call is refused with "unsupported channels" before any launch), or a stride other
 * than 1 or 2.  Arguments a call would refuse for another reason are not checked. */
#define LHN_KXK_F_DX    1   /* backward: dx != NULL */
#define LHN_KXK_F_DPOOL 2   /* backward: gy->dpool != NULL */
#define LHN_KXK_F_WT    4   /* wt_scratch != NULL: k_w_tapmajor re-lays the weights (backward: only ahead of a data gradient) */
#define LHN_KXK_SW_PLAIN0 1 /* LHN_PLAIN is set and does not start with '1' */
#define LHN_KXK_SW_PLAIN1 2 /* LHN_PLAIN=1 */
const char* lhn_conv_kxk_route(int backward, int N, int H, int W, int Cin, int Cout, int stride, int nrep, int features, int cus,
                               int switches);
/* out[i] = sum_r part[r*rep_stride + i]  (folds the replicated weight-gradient partials into the flat gradient) */
/* SyncBatchNorm (train/spawn_dist.py:37-38): run half-steps [step_begin, step_end) of a phase -- step 2*i = main
 * launches of op i, step 2*i+1 = the consumer of its statistics.  The caller all-reduces (SUM) the op's statistics
 * buffer between the two; count_scale = world size, pgrad_scale = 1/world (for d(gamma), d(beta)). */
int lhn_plan_run_range(void* plan, int phase, int64_t step_begin, int64_t step_end, void* workspace,
                       void* const* params, void* const* grads, void* const* io, int training, int grad_replicas,
                       int64_t grad_rep_stride, double count_scale, float pgrad_scale, void* stream);
/* SyncBatchNorm: stats[nrep][n] -> replica 0 holds the sum over the replicas, the others are zeroed; the caller then all-reduces
 * only the first n doubles (32x fewer bytes per BatchNorm than the replicated layout) and the finalize launches run unchanged. */
int lhn_fold_stat_replicas(double* stats, int64_t n, int nrep, void* stream);
int lhn_reduce_replicas(float* out, const float* part, int64_t n, int nrep, int64_t rep_stride, void* stream);
int lhn_ew_bwd(const lhn_view* srcs, int nsrc, const lhn_view* dst, const float* ddst, float out_slope,
               float* const* dsrcs, const int* accumulate, void* stream);
/* single-source form used by the plan: dst may carry a gate and a pooled gradient (channel attention) */
int lhn_ew_bwd2(const lhn_view* src, const lhn_view* dst, const float* ddst, const float* dst_dpool, float out_slope,
                float* dsrc, int accumulate, void* stream);
int lhn_maxpool2_bwd(const lhn_view* x, const lhn_view* y, const float* dy, float* dx, int dx_accumulate,
                     void* stream);
/* the same readers' backward kernels, also adding their part of the producer's BatchNorm-backward sums (lhn_bnsum; NULL = plain) */
int lhn_maxpool2_bwd2(const lhn_view* x, const lhn_view* y, const float* dy, float* dx, int dx_accumulate, const lhn_bnsum* bns,
                      void* stream);
int lhn_maxpool2_bwd3(const lhn_view* x, const lhn_view* y, const float* dy, float* dx, int dx_accumulate, const lhn_bnsum* bns,
                      const lhn_grad_adds* adds /*or NULL*/, void* stream);
int lhn_ew_bwd3(const lhn_view* src, const lhn_view* dst, const float* ddst, const float* dst_dpool, float out_slope, float* dsrc,
                int accumulate, const lhn_bnsum* bns, void* stream);
/* the same for 1..3 sources that all have dst's own geometry, in ONE pass over d(dst) / dst (residual sums); bns: per-source
 * lhn_bnsum pointers or NULL */
int lhn_ew_bwd_multi(const lhn_view* srcs, int nsrc, const lhn_view* dst, const float* ddst, const float* dst_dpool, float out_slope,
                     float* const* dsrcs, const int* accumulate, const lhn_bnsum* const* bns, void* stream);
/* 1 <= OH <= x.H and 1 <= OW <= x.W (the kernel visits the bins floor(h*OH/H) +- 1); out_cstride and out_coff are multiples of 4 */
int lhn_avgpool_bwd3(const lhn_view* x, const float* dout, int OH, int OW, int out_cstride, int out_coff, float* dx,
                     int dx_accumulate, const lhn_bnsum* bns, void* stream);
int lhn_conv_pw_bwd3(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, float* dbias, int stride, const float* dy_nchw, int nrep, int64_t rep_stride,
                     const lhn_pw_opts* opts, const lhn_bnsum* bns /*or NULL; stride 1, and a shape lhn_conv_pw_route has a kernel for*/, void* stream);
/* The two backward calls above with the BatchNorm-backward finalize of y taken in the kernel's prologue (lhn_bnbwdsrc; fin NULL =
 * the calls above).  gy->coef must point at the coefficient table: it is written.  lhn_conv_dw_bwd4 takes everything a depthwise
 * backward may carry: bns (the producer's sums of lhn_conv_dw_bwd2, x's first channel at bns->coff; NULL or bns->sums NULL: none),
 * the addends of lhn_conv_dw_bwd3, and fin; bns and addends exclude each other.
 * In-prologue fold: k_dw3_bwd_rows (3x3, stride 1, "same" padding, W >= 8; dilation 1 on maps of at most 256 pixels: the tile kernel
 * k_dwk_bwd_lds, same fold, LHN_DW_BWD_SMALL=0 keeps the row kernel) and k_pw_bwd_wr; every other kernel gets a lhn_bn_bwd_finalize2
 * launch in front, from this call (lhn_conv_dw_route / lhn_conv_pw_route name it where it is issued). */
int lhn_conv_dw_bwd4(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, int k, int stride, int pad, int dil, int nrep, int64_t rep_stride, const lhn_bnsum* bns,
                     const float* dx_add0, const float* dx_add1, const lhn_bnbwdsrc* fin, void* stream);
/* lhn_conv_dw_fwd3 / lhn_conv_pw_fwd2 with the BatchNorm finalize of x taken in the kernel's prologue (lhn_bnfinsrc; fin NULL = the
 * calls above).  One source only (no extra, no summed-on-load sources).  In-prologue fold: k_dwk_fwd_lds<3,1,1,true> (3x3, stride 1,
 * dilation 1, "same" padding, W >= 8), k_dws2_fwd_lds<true> (3x3, stride 2, pad 1), k_pw_fwd_wr<64, 2, 1, true> and
 * k_pw_fwd_wr<32, 1, 1, true> (the whole 1x1 in one register-W launch, Cin = 64 with 33..64 features or Cin = 32 with <= 32); every
 * other kernel gets a lhn_bn_finalize launch in front, from this call (lhn_conv_dw_route / lhn_conv_pw_route name it). */
int lhn_conv_dw_fwd4(const lhn_view* x, const float* w, const lhn_view* y, double* stats, int k, int stride, int pad, int dil,
                     const lhn_bnfin* fin, const lhn_view* extra, const float* coef2, const lhn_view* sum_out, const lhn_bnfinsrc* finsrc,
                     void* stream);
int lhn_conv_pw_fwd3(const lhn_view* x, const float* w, const float* bias, const lhn_view* y, double* stats, int stride,
                     float* y_nchw, const lhn_bnfin* fin, const lhn_pw_opts* opts, const lhn_bnfinsrc* finsrc, void* stream);
/* Which kernel lhn_conv_dw_fwd4 (backward = 0) / lhn_conv_dw_bwd4 (backward = 1) launches for this shape and feature set: host-only
 * (no device needed, nothing is launched), answered by the function the two calls themselves ask.  H, W, C are x's.
 * features: what the call carries.  switches: -1 = as this process read them from the environment, else a set of LHN_DW_SW_* bits.
 * Returns a static string (per thread, valid until the next call) in the spelling of profiles/dw_instances.md ("k_dw3_bwd_rows<1,BNS>
 * ps=2", "k_dw_bwd_data<7> + k_dw_bwd_weight<7,1> x 7", with "lhn_bn_bwd_finalize2 + " in front when the finalize takes its own
 * launch), or NULL when no kernel exists for the combination.  Arguments a call would refuse for another reason are not checked. */
#define LHN_DW_F_NO_WEIGHT 1   /* w (and dw) NULL: the k = 1 identity */
#define LHN_DW_F_EXTRA     2   /* forward: a second source */
#define LHN_DW_F_BNSUM     4   /* backward: the producer's BatchNorm sums */
#define LHN_DW_F_ADDS      8   /* backward: gradient addends */
#define LHN_DW_F_FIN       16  /* backward: a finalize source (lhn_bnbwdsrc) */
#define LHN_DW_F_NO_DX     32  /* backward: dx NULL */
#define LHN_DW_F_DX_ACC    64  /* backward: dx accumulated */
#define LHN_DW_F_FINSRC    128 /* forward: a finalize source (lhn_bnfinsrc); "lhn_bn_finalize + " in front where the kernel does not fold */
#define LHN_DW_SW_GATHER    1  /* LHN_DW_GATHER=1 */
#define LHN_DW_SW_BWD_V1    2  /* LHN_DW_BWD_V1=1 */
#define LHN_DW_SW_BWD_SMALL 4  /* the small-map route: set unless LHN_DW_BWD_SMALL=0 */
const char* lhn_conv_dw_route(int backward, int H, int W, int C, int k, int stride, int pad, int dil, int features, int switches);
int lhn_conv_pw_bwd4(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, float* dbias, int stride, const float* dy_nchw, int nrep, int64_t rep_stride,
                     const lhn_pw_opts* opts, const lhn_bnsum* bns, const lhn_bnbwdsrc* fin, void* stream);
/* Which kernels lhn_conv_pw_fwd2 (backward = 0) / lhn_conv_pw_bwd6 (backward = 1) launch for this shape and feature set, in order:
 * host-only (no device needed, nothing is launched), answered by the two functions the calls themselves ask (pw_fwd_route /
 * pw_bwd_route, csrc/k_conv_pw.hip).  N, H, W are x's; w_rows / w_cols: lhn_pw_opts' fields, 0 = Cout / Cin.  features: what the call
 * carries.  switches: -1 = as this process read them from the environment, else a set of LHN_PW_SW_* bits.
 * Returns a static string (per thread, valid until the next call): the template instances as a kernel trace prints them, joined
 * with " + ", " x n" behind a launch that repeats ("k_dy_inplace + k_pw_fwd_wr<256, 4, 1> x 2 + k_kxk_wgrad<128, 4, 1, true> x 2"),
 * with "lhn_bn_bwd_finalize2 + " in front, " + lhn_bn_finalize" or " + lhn_gate_bwd_reduce3" behind where the call issues that launch
 * itself; profiles/pw_instances.md is printed from it.  NULL: no kernel exists for the combination (the call is refused before any
 * launch), or the stride is not 1 or 2.  Other arguments a call would refuse for another reason are not checked. */
#define LHN_PW_F_NCHW      1     /* y_nchw / dy_nchw */
#define LHN_PW_F_STATS     2     /* forward: BatchNorm statistics */
#define LHN_PW_F_FUSE_FIN  4     /* forward: a fused finalize is asked for (lhn_bnfin) */
#define LHN_PW_F_EXTRA1    8     /* forward: one summed-on-load source */
#define LHN_PW_F_EXTRA2    16    /* forward: two */
#define LHN_PW_F_SUM_OUT   32    /* forward: sum_out */
#define LHN_PW_F_BNSUM     64    /* backward: reader-side BatchNorm sums (lhn_bnsum) */
#define LHN_PW_F_FIN       128   /* backward: a finalize source (lhn_bnbwdsrc) */
#define LHN_PW_F_GATESUM   256   /* backward: gate sums (lhn_gatesum) */
#define LHN_PW_F_NO_DX     512   /* backward: dx NULL */
#define LHN_PW_F_DX_ACC    1024  /* backward: dx accumulated (part of the call's description; no rule of the route reads it.  Behind the
                                    route, the launcher of the 32 -> 32 instances k_pw_bwd_wr<32, 32, 128, 2, false, BNS, *> sends an
                                    accumulating call to k_pw_bwd_wr<32, 32, 128, 3, false, BNS, 2>: the prior dx rides in the tile
                                    prefetch, same bits of dx.  The route's answer names the PF = 2 instance either way.
                                    LHN_PW_BWD_ACC_PREFETCH=0: the PF = 2 instance itself, dx re-read at the store) */
#define LHN_PW_F_DZ_DEAD   2048  /* backward: LHN_PW_BWD_DZ_DEAD */
#define LHN_PW_F_UNALIGNED 4096  /* a pointer the vector paths need at 16 bytes is not (forward: w, y_nchw; backward: dy_nchw, x's data),
                                    or the NCHW batch stride is no multiple of 4 floats */
#define LHN_PW_F_DBIAS     8192  /* backward: dbias given (an NCHW gradient's bias sums are a launch of their own on k_pw_bwd) */
#define LHN_PW_F_FINSRC    16384 /* forward: a finalize source (lhn_bnfinsrc); "lhn_bn_finalize + " in front where the kernel does not fold */
#define LHN_PW_SW_LDSW          1   /* LHN_PW_LDSW=1 */
#define LHN_PW_SW_K256          2   /* K = 256 in one pass: set unless LHN_PW_K256=0 */
#define LHN_PW_SW_BWD_NARROW    4   /* the narrow register-W backward: set unless LHN_PW_BWD_NARROW=0 */
#define LHN_PW_SW_BWD_SPLIT     8   /* LHN_PW_BWD_SPLIT=1 */
#define LHN_PW_SW_HEAD_STREAM   16  /* the streaming head kernels: set unless LHN_HEAD_STREAM=0 */
#define LHN_PW_SW_DETERMINISTIC 32  /* LHN_DETERMINISTIC=1 */
const char* lhn_conv_pw_route(int backward, int N, int H, int W, int Cin, int Cout, int stride, int w_rows, int w_cols, int features,
                              int switches);
int lhn_avgpool_bwd(const lhn_view* x, const float* dout /*[N,OH,OW,C]*/, int OH, int OW, float* dx,
                    int dx_accumulate, void* stream);
int lhn_gate_bwd_reduce(const lhn_view* y, const float* dz, float* dgate /*[N][C] dense*/, void* stream);
/* BatchNorm-backward sums of a GATED buffer without a pass of their own (the gate gradient needs one pass over (y, dz), the
 * pooled gradient of the attention exists only after it, and lhn_bn_bwd_reduce would be a second pass over both).  With
 *   du = (g[n,c] * dz + sum over the bins containing the pixel of e[n,bin,c]) * act'(u),   e = d loss / d pooled / |bin|
 * the sums split per sample:  sum du = sum_n (g * T0 + sum_bins e * M0),  sum du * xhat = sum_n (g * T1 + sum_bins e * M1)  with
 *   T0 = sum_px dz * act'(u), T1 = sum_px dz * act'(u) * xhat     per (n, c):      lhn_gate_bwd_reduce2 (tsum[N][2][C], = dgate + N*C)
 *   M0 = sum_{px in bin} act'(u), M1 = sum_{px in bin} act'(u) * xhat  per (n, bin, c): lhn_avgpool_fwd3 (pstat[N*9][2][C], forward)
 * and lhn_ca_mlp_bwd2 assembles them right where e is formed and stores them into replica 0 of the producers' sums.
 * slices: the (up to two) convolution + BatchNorm outputs that make up the buffer (common.py:40-66 gates cat(left, right)). */
typedef struct lhn_bn_slices {
  const float* save[2];   /* [2][C[k]] mean | invstd saved by lhn_bn_finalize                      */
  double*      sums[2];   /* [LHN_STAT_REPLICAS][2][C[k]] (zeroed by the caller) or NULL; lhn_ca_mlp_bwd2 only */
  int32_t      lo[2], C[2];
  int32_t      n;         /* 0..2 */
} lhn_bn_slices;
int lhn_gate_bwd_reduce2(const lhn_view* y, const float* dz, float* dgate /*[3][N][C]: dgate | tsum*/, float* tsum,
                         const lhn_bn_slices* slices, void* stream);
/* prezeroed != 0: dgate (and tsum) are already zero (the caller zeroes many such buffers with one memset) */
int lhn_gate_bwd_reduce3(const lhn_view* y, const float* dz, float* dgate, float* tsum, const lhn_bn_slices* slices, int prezeroed,
                         void* stream);
/* Gate-gradient sums of x's buffer from the backward of the heatmap head (litehourglass.py:159-166: the 128 -> 21 head is the only
 * reader of neck[1]'s gated buffer; common.py:40-66 is the attention whose gate it is).  The head's backward forms the complete dz
 * of that buffer (= its dx) in registers and holds the raw x for dW anyway, and dgate, T0, T1 are linear in dz -- so it adds, per
 * (image n, channel c of the buffer), with u = scale*raw + shift:
 *   dgate[n][c] += dx * act(u),   T0[n][c] += dx * act'(u),   T1[n][c] += dx * act'(u) * (raw - mean_c) * invstd_c
 * which is what lhn_gate_bwd_reduce3 leaves (same layout: dgate[N][cstride], tsum = dgate + N*cstride as [N][2][cstride], channels at
 * their index in the buffer; mean | invstd by the lhn_bn_slices rule, channels outside every slice use 0 and 1).  The buffers must be
 * zero before the call (the plan keeps them in the arena its backward zeroes).  The sums are those of the buffer only when this call's
 * dx is its whole gradient (no other reader); dx must be STORED: gs with dx_accumulate != 0 is refused.
 * lhn_conv_pw_bwd5 = lhn_conv_pw_bwd4 + gs (NULL: no sums).  The streaming head kernel k_head_bwd adds them in its own launch; where
 * it does not run (lhn_conv_pw_route: " + lhn_gate_bwd_reduce3") the call issues the lhn_gate_bwd_reduce3 launch itself behind its
 * kernels (x must then be the whole buffer): the result never depends on the kernel chosen. */
typedef struct lhn_gatesum {
  float*               dgate;    /* [3][N][cstride]: dgate | T0,T1 interleaved per image as [N][2][cstride] */
  const lhn_bn_slices* slices;   /* saved statistics of the buffer's BatchNorm slices (sums unused), or NULL */
} lhn_gatesum;
int lhn_conv_pw_bwd5(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, float* dbias, int stride, const float* dy_nchw, int nrep, int64_t rep_stride,
                     const lhn_pw_opts* opts, const lhn_bnsum* bns, const lhn_bnbwdsrc* fin, const lhn_gatesum* gs, void* stream);
/* lhn_conv_pw_bwd6 = lhn_conv_pw_bwd5 + flags (0 = lhn_conv_pw_bwd5).
 * LHN_PW_BWD_DZ_DEAD: the caller reads gy->dz (y's channels of the gradient buffer) no more after this call and does not expect
 * dy = d loss / d (convolution output) there either.  The wide register-W instances (lhn_conv_pw_route: k_pw_bwd_wr with a fifth
 * argument `true`) then run as their `false` twins, which keep dy in LDS and only READ dz: one write pass over the output's gradient
 * less.  Without the flag those shapes leave dy in place of dz, as the three-launch split path always did.  The flag is a permission,
 * not a request: the split path still forms dy in place and kernels that never stored it ignore it.  So with the flag the contents of
 * gy->dz after the call are
 * unspecified (dz or dy); dx, dW, dbias, the coefficients and every sum are the same bits either way in deterministic mode: the
 * result never depends on the flag or on the kernel chosen. */
#define LHN_PW_BWD_DZ_DEAD 1
int lhn_conv_pw_bwd6(const lhn_view* x, const float* w, const lhn_view* y, const lhn_gradview* gy, float* dx, int dx_accumulate,
                     float* dw, float* dbias, int stride, const float* dy_nchw, int nrep, int64_t rep_stride,
                     const lhn_pw_opts* opts, const lhn_bnsum* bns, const lhn_bnbwdsrc* fin, const lhn_gatesum* gs, int flags,
                     void* stream);
int lhn_avgpool_fwd3(const lhn_view* x, float* out /*[N,OH,OW,C]*/, int OH, int OW, float* pstat /*[N*OH*OW][2][C] or NULL*/,
                     const lhn_bn_slices* slices, void* stream);
/* H < 2 or W < 2 is refused: the segment layout of the pooled gradient needs two pixels per axis */
int lhn_ca_mlp_bwd2(const float* pooled, const float* w3, const float* gamma, const float* w1, const float* w2,
                    const float* dropmask, const float* save, const float* dgate, float* dpool, int cstride, int coff, int H,
                    int W, float* dw3, float* dgamma, float* dbeta, float* dw1, float* db1, float* dw2, float* db2, int N, int C,
                    int stage, double* gsum, double count_scale, float pgrad_scale, const float* tsum, const float* pstat,
                    const lhn_bn_slices* slices, void* stream);
/* ... and copy_src (or NULL): channels [0, copy_src->C) of the pooled buffer x have not been written yet -- they are the
 * pass-through half of a gated RepBasicUnit (litehourglass.py:74-77: ca(cat(left, conv(right)))).  The kernel takes their consumed
 * values from copy_src, pools them and stores them into x: no separate copy pass.  pstat may be NULL here. */
int lhn_avgpool_fwd4(const lhn_view* x, float* out, int OH, int OW, float* pstat, const lhn_bn_slices* slices,
                     const lhn_view* copy_src, void* stream);
int lhn_ca_mlp_bwd(const float* pooled, const float* w3, const float* gamma, const float* w1, const float* w2,
                   const float* dropmask, const float* save, const float* dgate, float* dpool /*[N,9,cs]*/,
                   int cstride, int coff, int H, int W, float* dw3, float* dgamma, float* dbeta, float* dw1,
                   float* db1, float* dw2, float* db2, int N, int C, int stage, double* gsum, double count_scale,
                   float pgrad_scale, void* stream);

/* CBAM (attention.py:269-294) between its `pre` convolutions and its final ReLU.  p = pre's output (its VALUE: raw + table), r =
 * residual_conv(x), out = relu(a * g * p + r) stored plain; g = sigmoid(W2 relu(W1 mean p) + W2 relu(W1 max p)) per (n, c), a =
 * sigmoid(conv7x7([mean_c, max_c](g p))) per pixel.  w1 [C/16, C], w2 [C, C/16], w7 [1, 2, 7, 7], no biases.  C % 16 == 0, C <= 256,
 * any N, H, W; anything else is refused before the first launch.  No float atomics: bitwise repeatable in every mode.
 * `save` (forward writes, backward reads) and `scratch` (backward only) are caller-owned float arrays; lhn_cbam_layout gives the
 * offsets in floats:  save_off[10] = avg[N][C], mx[N][C], argmax pixel (int32)[N][C], hidden rows after ReLU [N][2][C/16], g[N][C],
 * s[N][H][W][2], argmax channel (int32)[N][H][W], a[N][H][W], pooling partials, total;  scratch_off[8] = dq, dW7 partials, dg partials,
 * davg, dmx, dW1 partials, dW2 partials, total.
 * Backward: dout has out's geometry; dr is STORED with r's geometry; dp (p's geometry) receives d(loss)/d(value of p), STORED; dw1,
 * dw2, dw7 are ADDED to (one fold in fixed order each). */
int lhn_cbam_layout(int N, int H, int W, int C, int64_t* save_off /*[10]*/, int64_t* scratch_off /*[8]*/);
int lhn_cbam_fwd(const lhn_view* p, const lhn_view* r, const float* w1, const float* w2, const float* w7, const lhn_view* out,
                 float* save, void* stream);
int lhn_cbam_bwd(const lhn_view* p, const lhn_view* r, const float* w1, const float* w2, const float* w7, const lhn_view* out,
                 const float* dout, float* dp, float* dr, float* dw1, float* dw2, float* dw7, const float* save, float* scratch,
                 void* stream);

/* torch.optim.Adam (no amsgrad) over one flat fp32 parameter buffer -- the optimizer of dist_train.py:64-69 for the flat parameter
 * of litehandnet_amd.train.FlatParams: exp_avg / exp_avg_sq are the optimizer state of that one tensor, step = the 1-based count of
 * this update.  Buffers 16-byte aligned. */
int lhn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int64_t step, void* stream);

/* ---------------------------------------------------------------- pair launches
 * Two independent calls of one pool / combine / finalize entry in ONE launch (blockIdx.y selects the job; each job keeps the grid,
 * the replicas and the arithmetic of its single launch: every output is bit-identical to the two single calls, BatchNorm-backward
 * sums included wherever the single calls are run-to-run reproducible).  A job struct holds the arguments of the single entry named
 * in its comment, with the same meaning.  A pair entry refuses, before anything is launched and with the reason in
 * lhn_last_error(): whatever the single entry refuses for either job; jobs whose geometry differs (N, H, W, C, source count and
 * resolutions, pooled size); jobs whose outputs overlap (one base pointer and pixel stride: the channel ranges decide; otherwise
 * the address ranges); and the forms without a two-job kernel -- product / bilinear combines, SiLU / ReLU-sigmoid combine backward,
 * average pools with statistics or a copy source or on the small-bin kernel. */
typedef struct lhn_maxpool_job {          /* lhn_maxpool2_fwd (x, y) / lhn_maxpool2_bwd3 (all) */
  const lhn_view*      x;
  const lhn_view*      y;
  const float*         dy;
  float*               dx;
  int32_t              dx_accumulate;
  const lhn_bnsum*     bns;              /* or NULL */
  const lhn_grad_adds* adds;             /* or NULL */
} lhn_maxpool_job;
typedef struct lhn_ew_job {               /* lhn_ew_fwd3 (srcs .. mode) / lhn_ew_bwd3 (nsrc = 1) / lhn_ew_bwd_multi */
  const lhn_view*         srcs;
  int32_t                 nsrc;
  const float*            coef;          /* forward, or NULL */
  const lhn_view*         dst;
  float                   out_slope;
  int32_t                 mode;          /* forward */
  const float*            ddst;          /* backward from here on */
  const float*            dst_dpool;
  float* const*           dsrcs;         /* [nsrc] */
  const int*              accumulate;    /* [nsrc] */
  const lhn_bnsum* const* bns;           /* [nsrc] or NULL */
} lhn_ew_job;
typedef struct lhn_avgpool_job {          /* lhn_avgpool_fwd2; pstat / copy_src (lhn_avgpool_fwd4) are refused */
  const lhn_view*      x;
  float*               out;
  int32_t              OH, OW, out_cstride, out_coff;
  float*               pstat;
  const lhn_bn_slices* slices;
  const lhn_view*      copy_src;
} lhn_avgpool_job;
int lhn_maxpool2_fwd_pair(const lhn_maxpool_job* a, const lhn_maxpool_job* b, void* stream);
int lhn_maxpool2_bwd_pair(const lhn_maxpool_job* a, const lhn_maxpool_job* b, void* stream);
int lhn_ew_fwd_pair(const lhn_ew_job* a, const lhn_ew_job* b, void* stream);
int lhn_ew_bwd_pair(const lhn_ew_job* a, const lhn_ew_job* b, void* stream);
int lhn_ew_bwd_multi_pair(const lhn_ew_job* a, const lhn_ew_job* b, void* stream);
int lhn_avgpool_fwd_pair(const lhn_avgpool_job* a, const lhn_avgpool_job* b, void* stream);
/* lhn_bn_finalize2 for two separate BatchNorms.  Per job: the statistics, the lhn_bnfin slice (counter unused; C = the channels the
 * BatchNorm really has) and the channel stride of the statistics / save layout (>= C).  Tables, running statistics, saved
 * mean | invstd and num_batches_tracked of the two jobs must not overlap. */
int lhn_bn_finalize_pair(const double* stats_a, const lhn_bnfin* a, int stat_channels_a, const double* stats_b, const lhn_bnfin* b,
                         int stat_channels_b, int training, void* stream);

/* ---------------------------------------------------------------- plan executor
 * A plan is a static list of the calls above over one workspace arena, built by the Python
 * mirror of the reference's nn.Module tree (models/__init__.py:20-26 get_model).  One
 * lhn_plan_run() enqueues a whole forward (phase 0) or backward (phase 1) on the stream. */
typedef struct lhn_op {
  int32_t kind;
  int32_t in_buf[3], in_coff[3], in_C[3];
  int32_t reserved[6]; /* (round 2: deferred-finalize indices) */
  int32_t out_buf, out_coff, out_C;
  int32_t p[12];       /* parameter / state indices into the params array, -1 = none              */
  int64_t ws[12];      /* byte offsets into the workspace, -1 = none                               */
  int32_t i[8];
  float   f[8];        /* [0..3] op scalars (eps, momentum, slope, ..); [4..6] coefficients of summed input sources */
} lhn_op;

typedef struct lhn_buf {
  int64_t data_off, table_off, gate_off, grad_off, dpool_off, coef_off;  /* bytes, -1 = none */
  int32_t N, H, W, C;
} lhn_buf;

void* lhn_plan_create(const lhn_buf* bufs, int nbufs, const lhn_op* fwd, int nfwd, const lhn_op* bwd, int nbwd);
void  lhn_plan_destroy(void* plan);
/* Index of the backward op (a GATE_REDUCE) that a whole-plan run does NOT launch because the head's backward in front of it adds the
 * same sums (lhn_gatesum: the op before it is the backward of an NCHW 1x1 that stores the gradient of the whole gated buffer), or -1:
 * no such pair, LHN_HEAD_STREAM=0, or deterministic mode.  The op lists themselves are the same either way. */
int   lhn_plan_head_gate_fold(void* plan);
/* 1 when backward op bwd_index is the backward of an NHWC 1x1 whose output gradient no later op of the list touches (as a buffer's
 * gradient with overlapping channels, aliased buffers included, or through a byte offset): a whole-plan run then passes
 * LHN_PW_BWD_DZ_DEAD to lhn_conv_pw_bwd6 unless LHN_PW_BWD_DY_STORE=1; 0 otherwise; -1: index out of range.  The answer does not
 * depend on the switch, and the op lists are the same either way. */
int   lhn_plan_pw_dz_dead(void* plan, int bwd_index);
/* 1 when forward op fwd_index is a convolution + BatchNorm that hands its finalize to the next op of the list (a single-source NHWC
 * depthwise or 1x1 convolution over exactly the BatchNorm's output view, on a kernel that folds the statistics in its prologue:
 * lhn_bnfinsrc): a whole-plan training run then launches no lhn_bn_finalize for it.  0 otherwise, also with LHN_FWD_FIN_CONSUMER=0
 * or LHN_FUSE_FINALIZE=1; -1: index out of range.  The op lists are the same either way. */
int   lhn_plan_fwd_fin_consumer(void* plan, int fwd_index);
/* Pair launches of a whole-plan run (phase 0 = forward list, 1 = backward list): 1 when op `index` is the first op of a pair, 2 when
 * it is the second, 0 otherwise, also with LHN_PAIR_LAUNCH=0; -1: phase or index out of range.  Two kinds of pair:
 *   pool / combine: ops index and index + 1 of one kind and mode (MAXPOOL, plain AVGPOOL on the workgroup kernel, sum EW, MAXPOOL_BWD,
 *     leaky EW_BWD in its single- or multi-source form) with equal geometry, disjoint outputs (gradient buffers included, aliases too),
 *     neither reading what the other writes: the first op launches an lhn_*_pair entry, the second launches nothing;
 *   finalize (forward list, training and eval runs): two consecutive convolution + BatchNorm ops that both keep their separate
 *     lhn_bn_finalize launch (not handed to the next convolution, no LHN_FUSE_FINALIZE, no padded or twice-evaluated unit), the
 *     second convolution reading nothing of the first one's output: the first finalize waits and runs as job 0 of the second
 *     one's lhn_bn_finalize_pair.
 * lhn_plan_run_range never pairs.  The op lists are the same either way. */
int   lhn_plan_pair(void* plan, int phase, int index);
/* io: phase 0 {image NCHW, heatmap NCHW out}; phase 1 {image NCHW, d(heatmap) NCHW}.
 * training: a bit set -- bit 0 = train-mode BatchNorm (batch statistics, running statistics updated); bit 1 (LHN_RUN_TABLES_CURRENT,
 * eval only) = the workspace's per-buffer BatchNorm tables were built by an earlier eval run of THIS plan and no parameter
 * or running statistic changed since: the launches that only rebuild them are skipped. */
#define LHN_RUN_TABLES_CURRENT 2
/* bit 2: the launch sequence of this (phase, pointer set) may be captured into a hipGraph on its second sighting and replayed
 * afterwards (one graph launch instead of hundreds of kernel launches: Lite-HRNet runs 2,600 small launches per step and is
 * launch-bound).  Needs a real stream (the legacy default stream cannot be captured); a plan whose pointers never repeat
 * falls back to plain launches.  LHN_GRAPH=1 in the environment sets it for every call. */
#define LHN_RUN_GRAPH 4
int   lhn_plan_run(void* plan, int phase, void* workspace, void* const* params, void* const* grads,
                   void* const* io, int training, int grad_replicas, int64_t grad_rep_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
