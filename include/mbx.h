/* libmbx -- C-ABI boundary of the MI355X-native Multibox hot path.
 *
 * The reference (gvanhorn38/multibox, TF-0.11 Python) has no FFI of its own; its one
 * host-callback seam is tf.py_func(compute_assignments, ...) at loss.py:81-82 and the
 * numpy post-processing loop at detect.py:408-443.  Every entry point below names the
 * reference interface (file:line) it replaces.  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; device pointers unless marked HOST;
 *   - asynchronous on `stream` (a hipStream_t passed as void*), no allocation, no
 *     synchronisation, no global state: safe to capture into a hipGraph;
 *   - return 0 (MBX_OK) or a negative mbx_status; never throw across the boundary;
 *   - scratch memory comes from the caller; *_workspace_bytes() says how much.
 */
#ifndef MBX_H
#define MBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mbx_stream_t; /* hipStream_t */

typedef enum {
  MBX_OK = 0,
  MBX_ERR_INVALID_ARG = -1,
  MBX_ERR_UNSUPPORTED = -2,
  MBX_ERR_LAUNCH = -3,
  MBX_ERR_WORKSPACE = -4
} mbx_status;

int mbx_version(void);
const char* mbx_status_string(int status);

/* ---------------------------------------------------------------- priors (HOST)
 * Replaces priors.generate_priors (priors.py:185-314).  float64, bit-exact.
 * `grids` generalises the hard-coded [8,6,4,3,2,1] (priors.py:196); a grid of 1 gets
 * the single aspect-1 box (priors.py:206-258).  out = [rows,4] x1,y1,x2,y2.          */
int mbx_priors_count(int k, const int* grids, int n_grids);

/* CRC-32C (Castagnoli) of a host buffer, chained through `crc` (0 first): the checksum of TFRecord frames
 * (inputs.py:225-247 reads them with tf.TFRecordReader) and of TF checkpoint table blocks (train.py:15-90). Host code. */
uint32_t mbx_crc32c(const void* data, uint64_t n, uint32_t crc);
int mbx_generate_priors(const double* aspect_ratios, int k, double min_scale, double max_scale,
                        int restrict_to_image_bounds, const int* grids, int n_grids,
                        double* out /*HOST [rows,4]*/);

/* ------------------------------------------------------- decode + confidences (K12)
 * loss.py:67-74: decoded = raw_locs + tile(priors); conf = sigmoid(logits) + eps_add.
 * (model.py:322 applies the sigmoid; eps_add = 1e-10 for the loss, 0 for detect.)
 * Any output pointer may be NULL.                                                     */
int mbx_decode_conf(const float* raw_locs /*[B,P,4]*/, const float* logits /*[B,P]*/,
                    const float* priors /*[P,4]*/, int B, int P, float eps_add,
                    float* decoded /*[B,P,4]*/, float* conf /*[B,P]*/, mbx_stream_t stream);

/* ------------------------------------------------------------------ matching (A6)
 * Replaces the tf.py_func(compute_assignments) callback (loss.py:8-53, 81-82).
 * Inputs exactly as the callback receives them: prior-decoded locations, confidences
 * with 1e-10 already added, zero-padded gt, counts.  Per image: cost
 * C[p,j] = (alpha/2)*||l_p - g_j||^2 - log c_p + log(1-c_p) built in float32 in the
 * reference's operation order (loss.py:21-35), solved as a rectangular linear sum
 * assignment in float64 (shortest augmenting path; scipy's linear_sum_assignment,
 * loss.py:40).  match[b,p] = gt index or -1; the reference's 0/1 partition and
 * row-ordered stacked_gt (loss.py:44-48) follow from it.
 * status[b]: 0 ok, 1 n_gt > P or n_gt > G (infeasible), 2 a non-finite location or log-confidence, or no assignment of
 * finite cost (scipy raises there); n_gt <= 0: status 0, nothing matched.  Where status[b] != 0 the row of `match` is all -1.
 * Rows j >= n_gt[b] of `gt` are padding and never read.  A cost that overflows float32 to +inf is a legal entry, as for scipy.
 * Among assignments of equal total cost the choice is the kernel's own (shortest augmenting path; among equal candidates
 * a free prediction first, then the lowest index) and may differ from scipy's; it is the same on every call and does not
 * depend on B or on the image's place in the launch.  P and G are limited by 36 P + 16 G + 16 <= 150 KiB of LDS (P = 4221
 * at G = 100), above: MBX_ERR_UNSUPPORTED, nothing launched or written.                                                */
size_t mbx_match_workspace_bytes(int B, int P, int G);
int mbx_match(const float* decoded /*[B,P,4]*/, const float* conf /*[B,P]*/,
              const float* gt /*[B,G,4]*/, const int32_t* n_gt /*[B]*/, float alpha,
              int B, int P, int G, int32_t* match /*[B,P]*/, int32_t* status /*[B]*/,
              void* workspace, size_t workspace_bytes, mbx_stream_t stream);

/* THRESHOLD MATCHING behind mbx_match (SSD, Liu et al. 2016, section 2.2, "matching strategy"; optional, not in the
 * reference, off unless the caller asks).  mbx_match is bipartite: every box gets exactly one prior.  This step then gives
 * every prior that is still free to the box it overlaps most, if that overlap is over a threshold, so that priors which sit
 * squarely on an object are trained as positives and not as background.  `priors` are the PRIORS themselves as corners
 * (x1, y1, x2, y2), not the decoded predictions; `match` is mbx_match's output and is updated in place.  Per image b, with
 * n = n_gt[b]:
 *   status[b] != 0 or n <= 0 (or n > G, which mbx_match never leaves with status 0): the image is SKIPPED, its row of
 *   `match` stays byte for byte as it was and n_extra[b] = 0.
 *   Otherwise, for every prior p with match[b,p] < 0 and every box j in [0, n): the IoU in float64 on the float32 inputs
 *   widened to double, in this term order (the prior first):
 *     iw = min(p.x2, j.x2) - max(p.x1, j.x1), ih likewise;  inter = iw > 0 && ih > 0 ? iw * ih : 0
 *     area = (x2 - x1) * (y2 - y1);  uni = area_p + area_j - inter;  iou = uni > 0 ? inter / uni : 0
 *   best_j = the j with the largest iou, the lowest such j among equals.  If iou(p, best_j) > (double)iou_threshold --
 *   strictly -- match[b,p] = best_j.  (An IoU that is NaN, which takes a non-finite prior, is over no threshold.)
 *   A prior that mbx_match assigned keeps its box, even where another box overlaps it more.  Rows j >= n of `gt` are
 *   padding and are never read: a NaN there changes nothing.
 *   n_extra[b] = the number of priors newly assigned in image b.  Every n_extra[b] is written on every call (no memset by
 *   the caller); n_extra may be NULL.
 * An image's row depends on its own inputs only -- not on B or its place in the launch -- and the same input gives the same
 * bytes on every call (no floating-point atomics, the count is a wave and LDS reduction).  With iou_threshold = 1.0f no IoU
 * can exceed it: `match` comes back byte-identical and n_extra all zero.
 * NULL priors / gt / n_gt / status / match, B < 0, P <= 0, G <= 0 or an iou_threshold not in (0, 1] (NaN included):
 * MBX_ERR_INVALID_ARG; G > 1536 (the staged boxes, 40 bytes each, would not fit the LDS of a plain launch):
 * MBX_ERR_UNSUPPORTED; nothing is launched or written either way.  B == 0: MBX_OK.  One launch on `stream`, one workgroup
 * per image, no workspace, graph-capturable.  mbx_loss_fwd_bwd and mbx_loss_fwd_bwd_mined read the extended `match` as
 * they read any other; mining counts its positives from it, so its budget grows with the priors added here.
 * What threshold matching does to AP on real data is NOT measured here: no trained model or dataset is at hand.          */
int mbx_match_extend(const float* priors /*[P,4] x1,y1,x2,y2*/, const float* gt /*[B,G,4]*/,
                     const int32_t* n_gt /*[B]*/, const int32_t* status /*[B], as mbx_match left it*/,
                     float iou_threshold, int B, int P, int G,
                     int32_t* match /*[B,P] IN/OUT: mbx_match's output*/,
                     int32_t* n_extra /*[B] or NULL*/, mbx_stream_t stream);

/* ATSS MATCHING behind mbx_match (Adaptive Training Sample Selection, Zhang et al., CVPR 2020; optional, not in the
 * reference, off unless the caller asks; the alternative to mbx_match_extend -- a caller runs one of the two).  Instead of
 * one hand-picked IoU number every box gets a threshold of its own from the priors around it.  `priors` are the priors as
 * corners, `match` is mbx_match's output and is updated in place, as for mbx_match_extend.  The priors are described in
 * pyramid LEVELS: level_start[0 .. n_levels], a HOST array read at the call and handed to the kernel by value, with
 * level_start[0] = 0, strictly ascending, level_start[n_levels] = P; level l holds priors [level_start[l], level_start[l+1]).
 * All arithmetic is float64 on the float32 inputs widened to double, in exactly this order, no product fused into a sum.
 * Per image b, with n = n_gt[b]:
 *   status[b] != 0, n <= 0 or n > G: the image is SKIPPED, its row of `match` stays byte for byte as it was,
 *   n_extra[b] = 0 and thr[b, :] = 0.0 (mbx_match_extend's skip rule).
 *   Centres, of priors and boxes alike:  cx = (x1 + x2) * 0.5,  cy = (y1 + y2) * 0.5.
 *   Distance of box j < n and prior p:  dx = cx_p - cx_j,  dy = cy_p - cy_j,  d2 = dx * dx + dy * dy.
 *   CANDIDATES of box j: on every level the min(topk, level size) priors with the smallest d2; equal d2 goes to the lowest
 *   prior index; a NaN d2 ranks behind every number, +inf included, by index among NaNs.  m = sum over the levels of
 *   min(topk, size_l) is the same for every box of a call.
 *   IoU of a candidate: mbx_match_extend's, term by term, the prior first.
 *   THRESHOLD of box j, over its m candidate IoUs taken in ascending prior index, each sum starting from 0.0:
 *     mean = (sum iou) / m;   var = (sum (iou - mean) * (iou - mean)) / (m - 1);   std = sqrt(var), 0.0 when m == 1;
 *     thr_j = mean + std
 *   (the sample standard deviation, as in the authors' code).  Every candidate counts: those mbx_match assigned and those
 *   with IoU 0 too.
 *   A candidate p is a POSITIVE of j iff  iou > 0  and  iou >= thr_j (not strict; a NaN fails it)  and the prior's centre is
 *   strictly inside the box:  x1_j < cx_p && cx_p < x2_j && y1_j < cy_p && cy_p < y2_j.
 *   ASSIGNMENT: every prior with match[b,p] < 0 that is a positive of at least one box gets the box of the largest IoU, the
 *   lowest j among equals.  A prior that mbx_match assigned keeps its box.  Rows j >= n of `gt` are never read.
 *   n_extra[b] = the number of priors newly assigned;  thr[b,j] = thr_j for j < n and 0.0 for j >= n.  Each may be NULL;
 *   every element is written on every call (no memset by the caller).
 * An image's row depends on its own inputs only -- not on B or its place in the launch -- and the same input gives the same
 * bytes on every call: no floating-point atomics; the claims are resolved by an unsigned 64-bit max on IoU bit patterns in
 * LDS and an unsigned integer min on `match`, neither of which depends on the order of arrival.
 * With k priors per cell sharing one centre, topk = 9 reaches about 9 / k cells of a level (about two at k = 5): a caller who
 * wants the paper's nine LOCATIONS passes 9 * k.
 * NULL priors / level_start / gt / n_gt / status / match, B < 0, P <= 0, G <= 0, topk < 1, n_levels outside [1, 8] or a
 * level_start that does not start at 0, is not strictly ascending or does not end at P: MBX_ERR_INVALID_ARG.  The launch
 * holds an image in the LDS of a plain launch:
 *     8 P + 40 G + 2 G m + 8 W m + 128  <=  65536 bytes,   W = the most of 16, 8, 4, 2, 1 wavefronts that fits,  and P < 65535;
 * a size with no such W: MBX_ERR_UNSUPPORTED.  (P = 4221, G = 100, six levels, topk = 9 -- m <= 54 -- needs 54 KB at W = 16;
 * P = 646, G = 13 fits at every topk.)  Nothing is launched or written for either error.  B == 0: MBX_OK.
 * mbx_match_atss_supported gives the same verdict for a size, on a host without a GPU too.  No environment variable is read.
 * One launch on `stream`, one workgroup per image, no workspace, graph-capturable (level_start is not read after the call
 * returns).  The four loss entries read the extended `match` as they read any other; mining counts its positives from it.
 * What ATSS does to AP on real data is NOT measured here: no trained model or dataset is at hand.                         */
int mbx_match_atss_supported(int P, int G, int n_levels, const int32_t* level_start /*HOST [n_levels+1]*/, int topk);
int mbx_match_atss(const float* priors /*[P,4] x1,y1,x2,y2*/, const int32_t* level_start /*HOST [n_levels+1]*/,
                   int n_levels, const float* gt /*[B,G,4]*/, const int32_t* n_gt /*[B]*/,
                   const int32_t* status /*[B], as mbx_match left it*/, int topk, int B, int P, int G,
                   int32_t* match /*[B,P] IN/OUT: mbx_match's output*/, int32_t* n_extra /*[B] or NULL*/,
                   double* thr /*[B,G] or NULL*/, mbx_stream_t stream);

/* TASK-ALIGNED MATCHING behind mbx_match (the Task-Aligned Assigner of TOOD, Feng et al., ICCV 2021, also the assigner of
 * PP-YOLOE, YOLOv6 and YOLOv8; optional, not in the reference, off unless the caller asks; the alternative to
 * mbx_match_extend and mbx_match_atss -- a caller runs one of the three).  Those two promote a free prior by what the PRIORS
 * overlap; this one looks at what the network currently PREDICTS: per box it picks the priors whose prediction is already
 * both confident and well placed, ranked by t = s^alpha * u^beta, s the score and u the IoU of the decoded prediction with
 * the box.  `priors` are the priors as corners, `decoded` [B,P,4] and `conf` [B,P] are what mbx_match reads (the decoded
 * predictions as corners, sigmoid + 1e-10), `match` is mbx_match's output and is updated in place.  alpha = alpha_halves / 2
 * (an integer number of halves in [0, 8], so the power needs products and one square root only), beta an integer in [1, 16];
 * the paper's setting is topk 13, alpha 1 (alpha_halves 2), beta 6.
 * All arithmetic is float64 on the float32 inputs widened to double, in exactly this order, no product fused into a sum.
 * Per image b, with n = n_gt[b]:
 *   status[b] != 0, n <= 0 or n > G: the image is SKIPPED, its row of `match` stays byte for byte as it was,
 *   n_extra[b] = 0 and thr[b, :] = 0.0 (mbx_match_extend's skip rule).
 *   Score of prior p:  s = (double)conf[b,p].
 *   Overlap of prior p and box j < n:  u = mbx_match_extend's IoU, term by term, with e = decoded[b,p] first and the box second:
 *     iw = min(e.x2, j.x2) - max(e.x1, j.x1), ih likewise;  inter = iw > 0 && ih > 0 ? iw * ih : 0
 *     area = (x2 - x1) * (y2 - y1);  uni = area_e + area_j - inter;  u = uni > 0 ? inter / uni : 0
 *   The corners are used as they are, nothing is put in order first (as mbx_match_ignore with per_image).
 *   Metric:  r = 1.0; alpha_halves / 2 times: r = r * s;  if alpha_halves is odd: r = r * sqrt(s) (correctly rounded);
 *            w = 1.0; beta times: w = w * u;   t = r * w.
 *   CANDIDATES of box j: every prior p whose own centre -- of the PRIOR, cx = (x1 + x2) * 0.5, cy = (y1 + y2) * 0.5 from
 *   `priors` -- lies strictly inside the box, x1_j < cx && cx < x2_j && y1_j < cy && cy < y2_j (mbx_match_atss's expressions
 *   and comparisons), and whose t > 0 (a NaN fails).  Priors that mbx_match assigned count as candidates like any other.
 *   SELECTION: the min(topk, number of candidates) candidates with the largest t; equal t goes to the lowest prior index.
 *   thr[b,j] = the t of the last one selected, 0.0 where the box has no candidate, and 0.0 for j >= n.
 *   ASSIGNMENT: every prior with match[b,p] < 0 that at least one box selected gets the box of the largest u, the lowest j
 *   among equals.  A prior with match[b,p] >= 0 keeps its box.  Rows j >= n of `gt` are never read.
 *   n_extra[b] = the number of priors newly assigned.  n_extra and thr may each be NULL; every element is written on every
 *   call (no memset by the caller).
 * An image's row depends on its own inputs only -- not on B or its place in the launch -- and the same input gives the same
 * bytes on every call: no floating-point atomics; the claims are resolved as mbx_match_atss resolves them, by an unsigned
 * 64-bit max on the bit patterns of u in LDS and an unsigned integer min on `match`, neither of which depends on the order of
 * arrival.
 * The bipartite match stays in front: every box keeps its one guaranteed prior, and that is what carries training while the
 * predictions still overlap nothing -- this call then adds nothing.  TOOD's normalised soft target (t scaled per box to the
 * largest IoU) is NOT part of this entry: mbx_loss_fwd_bwd_quality supplies an IoU target for the confidence.
 * NULL priors / decoded / conf / gt / n_gt / status / match, B < 0, P <= 0, G <= 0, topk < 1, alpha_halves outside [0, 8] or
 * beta outside [1, 16]: MBX_ERR_INVALID_ARG.  The launch holds an image in the LDS of a plain launch:
 *     8 P + 40 G + 64 + 2 G m  <=  65536 bytes,   m = min(topk, P),   and P < 65535
 * (the claims, the staged boxes, the wavefronts' counts, the selected priors of every box as 2-byte indices); any other
 * size: MBX_ERR_UNSUPPORTED.  (P = 4221, G = 100, topk = 13 needs 40 KB; P = 646, G = 13 fits at every topk.)  Nothing is
 * launched or written for either error.  B == 0: MBX_OK.  mbx_match_tal_supported gives the same verdict for a size, on a
 * host without a GPU too.  No environment variable is read.  One launch on `stream`, one workgroup per image of min(G, 16)
 * wavefronts, a wavefront per box, no workspace, graph-capturable.  The loss entries read the extended `match` as they read
 * any other; mining counts its positives from it; mbx_match_ignore may run behind it.
 * What task-aligned matching does to AP on real data is NOT measured here: no trained model or dataset is at hand.         */
int mbx_match_tal_supported(int P, int G, int topk);
int mbx_match_tal(const float* priors /*[P,4] x1,y1,x2,y2*/, const float* decoded /*[B,P,4], as mbx_match reads them*/,
                  const float* conf /*[B,P] sigmoid + 1e-10, as mbx_match reads it*/, const float* gt /*[B,G,4]*/,
                  const int32_t* n_gt /*[B]*/, const int32_t* status /*[B], as mbx_match left it*/, int topk,
                  int alpha_halves /*alpha = alpha_halves / 2, in [0, 8]*/, int beta /*[1, 16]*/, int B, int P, int G,
                  int32_t* match /*[B,P] IN/OUT: mbx_match's output*/, int32_t* n_extra /*[B] or NULL*/,
                  double* thr /*[B,G] or NULL*/, mbx_stream_t stream);

/* IGNORE BAND behind the matching (RetinaNet, Lin et al. 2017: positive at or over 0.5, negative under 0.4, neither in
 * between; Faster R-CNN's RPN and SSD derivatives likewise, YOLOv3 by the prediction's overlap; optional, not in the
 * reference, off unless the caller asks).  A prior that sits on an object but is not the one the matcher picked is not
 * background: it gets a third state, MBX_MATCH_IGNORED, and mbx_loss_fwd_bwd_ignore leaves it out of the confidence loss.
 * Runs behind mbx_match, and behind mbx_match_extend or mbx_match_atss when one of them runs; `match` is their output and is
 * updated in place.  `boxes` are what the overlap is judged by, as corners (x1, y1, x2, y2):
 *   per_image == 0: [P,4], the PRIORS themselves, shared by all images;
 *   per_image != 0: [B,P,4], image b reads its own row -- a caller passes the decoded predictions here (YOLOv3's rule).  The
 *   formula is applied to the corners as they are, nothing is put in order first: a degenerate or non-finite prediction is
 *   whatever the formula and the comparisons below make of it.
 * Per image b, with n = n_gt[b]:
 *   status[b] != 0, n <= 0 or n > G: the image is SKIPPED, its row of `match` stays byte for byte as it was and
 *   n_ignored[b] = 0 (mbx_match_extend's skip rule).
 *   Otherwise, for every prior p with match[b,p] == MBX_MATCH_FREE (-1) exactly, e its box, and the boxes j in [0, n): the IoU
 *   in float64 on the float32 inputs widened to double, mbx_match_extend's formula term by term, e first:
 *     iw = min(e.x2, j.x2) - max(e.x1, j.x1), ih likewise;  inter = iw > 0 && ih > 0 ? iw * ih : 0
 *     area = (x2 - x1) * (y2 - y1);  uni = area_e + area_j - inter;  iou = uni > 0 ? inter / uni : 0
 *   If iou >= (double)iou_threshold -- NOT strict -- for any j, match[b,p] = MBX_MATCH_IGNORED (-2).  Only whether some box
 *   reaches the threshold matters, so the walk over j stops at the first that does.  A NaN IoU passes nothing.
 *   The quotient is the float64 inter / uni that mbx_match_extend compares: with the priors as `boxes`, `> hi` there and
 *   `>= lo` here (lo <= hi) split the free priors without a gap or an overlap -- every prior that mbx_match_extend left
 *   free and whose largest IoU lies in [lo, hi] is ignored, and none that it took.
 *   A prior with match >= 0 keeps its box and one with match <= -2 its value: a second call changes nothing.  Rows j >= n of
 *   `gt` are padding and are never read: a NaN there changes nothing.
 *   n_ignored[b] = the number of priors newly ignored in image b.  Every n_ignored[b] is written on every call (no memset by
 *   the caller); n_ignored may be NULL.
 * An image's row depends on its own inputs only -- not on B or its place in the launch -- and the same input gives the same
 * bytes on every call (no floating-point atomics, the count is a wave and LDS reduction).
 * NULL boxes / gt / n_gt / status / match, B < 0, P <= 0, G <= 0 or an iou_threshold not in (0, 1] (NaN included):
 * MBX_ERR_INVALID_ARG; G > 1536 (the staged boxes, 40 bytes each, would not fit the LDS of a plain launch):
 * MBX_ERR_UNSUPPORTED; nothing is launched or written either way.  B == 0: MBX_OK.  One launch on `stream`, one workgroup
 * per image, no workspace, graph-capturable.
 * The five loss entries from before the band read a negative `match` as a negative, -2 included: a caller that runs this
 * uses mbx_loss_fwd_bwd_ignore.
 * What the band does to AP on real data is NOT measured here: no trained model or dataset is at hand.                     */
enum { MBX_MATCH_FREE = -1, MBX_MATCH_IGNORED = -2 };
int mbx_match_ignore(const float* boxes /*[P,4], or [B,P,4] when per_image*/, int per_image,
                     const float* gt /*[B,G,4]*/, const int32_t* n_gt /*[B]*/,
                     const int32_t* status /*[B], as mbx_match left it*/, float iou_threshold, int B, int P, int G,
                     int32_t* match /*[B,P] IN/OUT*/, int32_t* n_ignored /*[B] or NULL*/, mbx_stream_t stream);

/* ---------------------------------------------------------------- loss fwd+bwd (A7)
 * loss.py:88-101 given the matching: loc_loss = alpha * 1/2 sum (decoded-gt)^2 over
 * matched rows; conf_loss = -sum log(c_matched) - sum log(1 - c_unmatched + 1e-10),
 * c = sigmoid(logit) + 1e-10.  Also the gradients w.r.t. raw_locs and the logits (no
 * gradient through the matching: py_func, loss.py:82).  loss2 = {loc_loss, conf_loss}.
 * grad_scale multiplies both gradients (1 for the reference's batch-sum loss).
 * conf_is_logit = 1: `conf_in` holds logits (gradient goes through the sigmoid of
 * model.py:322); 0: `conf_in` holds sigmoid outputs as loss.add_loss receives them
 * (d_logits then is the gradient w.r.t. those confidences).                           */
size_t mbx_loss_workspace_bytes(int B);
int mbx_loss_fwd_bwd(const float* decoded /*[B,P,4]*/, const float* conf_in /*[B,P]*/,
                     int conf_is_logit, const float* gt /*[B,G,4]*/,
                     const int32_t* match /*[B,P]*/, float alpha, float grad_scale, int B, int P,
                     int G, float* loss2 /*[2]*/,
                     float* d_raw_locs /*[B,P,4] or NULL*/, float* d_logits /*[B,P] or NULL*/,
                     void* workspace, size_t workspace_bytes, mbx_stream_t stream);

/* mbx_loss_fwd_bwd with HARD-NEGATIVE MINING (SSD, Liu et al. 2016, section 2.2; optional, not in the reference, off unless
 * the caller asks): per image only the highest-scoring negatives count, a fixed number per positive; the others contribute
 * neither loss nor gradient.  Every argument up to d_logits is mbx_loss_fwd_bwd's, same order and meaning.  Per image b:
 *   n_pos = number of p with match[b,p] >= 0;  N_neg = P - n_pos
 *   K     = min(N_neg, max(min_neg, neg_per_pos * n_pos)), the product in 64 bits: integer arithmetic, exact
 *   the candidates are the negatives (match[b,p] < 0), ordered by the order-preserving image of conf_in[b,p] -- THE FLOAT
 *   PASSED IN: the logit when conf_is_logit = 1, the confidence otherwise; both are monotone in the negative's loss, and the
 *   order then does not depend on the device's expf / logf -- descending, bit-equal images by ascending p.  It is the image
 *   mbx_decode_filter_topk sorts by: -0 == +0, a NaN ranks first (a NaN negative is taken whenever K > 0 and makes
 *   conf_loss NaN, as in mbx_loss_fwd_bwd).  The first K candidates are SELECTED;  n_neg[b] = K (n_neg may be NULL).
 * Positives and selected negatives get exactly the terms and gradients of mbx_loss_fwd_bwd.  An unselected negative adds
 * nothing to conf_loss and its d_logits is +0.0f.  d_raw_locs and loss2[0] do not depend on the selection.  Nothing is
 * normalised by n_pos: the loss stays a batch sum and grad_scale the caller's.
 * If K == N_neg for every image (min_neg >= P, say), loss2, d_raw_locs and d_logits are byte-identical to
 * mbx_loss_fwd_bwd on the same inputs (same per-thread stride, same reduction order).  An image's outputs depend on its
 * own row only -- not on B or its place in the launch -- and the same input gives the same bytes on every call (no
 * floating-point atomics).  No limit on P: the K-th candidate is found by a radix select over the row, not by a sort.
 * neg_per_pos < 1, min_neg < 0 or anything mbx_loss_fwd_bwd rejects: MBX_ERR_INVALID_ARG; workspace_bytes <
 * mbx_loss_mined_workspace_bytes(B, P): MBX_ERR_WORKSPACE; nothing is launched or written either way.  Two launches on
 * `stream`, one workgroup per image.
 * What mining does to AP on real data is NOT measured here: no trained model or dataset is at hand.                  */
size_t mbx_loss_mined_workspace_bytes(int B, int P);
int mbx_loss_fwd_bwd_mined(const float* decoded /*[B,P,4]*/, const float* conf_in /*[B,P]*/,
                           int conf_is_logit, const float* gt /*[B,G,4]*/,
                           const int32_t* match /*[B,P]*/, float alpha, float grad_scale, int B, int P,
                           int G, float* loss2 /*[2]*/,
                           float* d_raw_locs /*[B,P,4] or NULL*/, float* d_logits /*[B,P] or NULL*/,
                           int neg_per_pos, int min_neg, int32_t* n_neg /*[B] or NULL*/,
                           void* workspace, size_t workspace_bytes, mbx_stream_t stream);

/* mbx_loss_fwd_bwd with the FOCAL LOSS on the confidence term (Lin et al. 2017, "Focal Loss for Dense Object Detection";
 * optional, not in the reference, off unless the caller asks): every prior stays in the loss and the well-classified ones are
 * down-weighted by (1 - p_t)^gamma, with a class weight on each side.  Every argument up to d_logits is mbx_loss_fwd_bwd's,
 * same order and meaning.  Per prior, in float32 and in mbx_loss_fwd_bwd's operation order:
 *   s = sigmoid(conf_in) when conf_is_logit, else conf_in;   c = s + 1e-10f;   w = (1 - c) + 1e-10f
 *   ds = s (1 - s) when conf_is_logit, else 1
 * and then
 *   positive (match >= 0):  term L = -w_pos * w^gamma * log c     dL/ds = w_pos * (gamma * w^(gamma-1) * log c - w^gamma / c)
 *   counted negative:       term L = -w_neg * c^gamma * log w     dL/ds = w_neg * (c^gamma / w - gamma * c^(gamma-1) * log w)
 *   d_logits = dL/ds * ds * grad_scale;   loss2[1] = the sum of the terms, accumulated in double.
 * With gamma == 0 the gamma * x^(gamma-1) * log term is left out, not multiplied by zero.  Both gradient brackets are sums
 * of same-sign terms: nothing cancels.  With s exactly 0 or 1 the epsilons keep c, w >= 1e-10, so every term and gradient
 * is finite for gamma in [0, 10], gamma < 1 included.  The paper's alpha is w_pos = alpha, w_neg = 1 - alpha (0.25 with
 * gamma = 2).  The location loss, d_raw_locs and loss2[0] are mbx_loss_fwd_bwd's, untouched.  Nothing is normalised by
 * the number of positives: the loss stays a batch sum and grad_scale the caller's.  A conf_in outside [0, 1] with
 * conf_is_logit = 0, or a NaN, gives whatever IEEE arithmetic gives, as in mbx_loss_fwd_bwd.
 * Which negatives are counted:
 *   neg_per_pos == 0: every negative; min_neg must be 0; n_neg[b] = P - n_pos (n_neg may be NULL).
 *   neg_per_pos >= 1: exactly the selection of mbx_loss_fwd_bwd_mined -- the same key on conf_in, the same K, the same
 *   ties, n_neg[b] = K.  The focal negative term is increasing in c, so the highest score is still the highest loss.  An
 *   unselected negative adds nothing to conf_loss and its d_logits is +0.0f.
 * gamma == 0 && w_pos == 1 && w_neg == 1 gives loss2, d_raw_locs and d_logits byte-identical to mbx_loss_fwd_bwd
 * (neg_per_pos == 0) and to mbx_loss_fwd_bwd_mined with the same neg_per_pos / min_neg (neg_per_pos >= 1): same per-thread
 * stride, same reduction order, and x * 1.0f is exact.  An image's outputs depend on its own row only -- not on B or its
 * place in the launch -- and the same input gives the same bytes on every call (no floating-point atomics).  Any P.
 * gamma not in [0, 10] (NaN included), a weight that is negative or not finite, neg_per_pos < 0, min_neg < 0, min_neg > 0
 * with neg_per_pos == 0, or anything mbx_loss_fwd_bwd rejects: MBX_ERR_INVALID_ARG; workspace_bytes <
 * mbx_loss_focal_workspace_bytes(B, P): MBX_ERR_WORKSPACE; nothing is launched or written either way.  Two launches on
 * `stream`, one workgroup per image, graph-capturable.
 * What the focal loss does to AP on real data is NOT measured here: no trained model or dataset is at hand.            */
size_t mbx_loss_focal_workspace_bytes(int B, int P);
int mbx_loss_fwd_bwd_focal(const float* decoded /*[B,P,4]*/, const float* conf_in /*[B,P]*/,
                           int conf_is_logit, const float* gt /*[B,G,4]*/,
                           const int32_t* match /*[B,P]*/, float alpha, float grad_scale, int B, int P,
                           int G, float* loss2 /*[2]*/,
                           float* d_raw_locs /*[B,P,4] or NULL*/, float* d_logits /*[B,P] or NULL*/,
                           float gamma, float w_pos, float w_neg,
                           int neg_per_pos /*0 = every negative counts*/, int min_neg, int32_t* n_neg /*[B] or NULL*/,
                           void* workspace, size_t workspace_bytes, mbx_stream_t stream);

/* mbx_loss_fwd_bwd_focal with a CHOICE OF LOCATION TERM (optional, not in the reference, off unless the caller asks): the
 * one entry for every combination of location term, focal loss and mining.  Every argument but loc_type and loc_beta is
 * mbx_loss_fwd_bwd_focal's, same order and meaning; gamma == 0 with weights (1, 1) is the plain confidence term,
 * neg_per_pos != 0 mines.  The confidence side (loss2[1], d_logits, n_neg) does not depend on loc_type.
 * Per positive prior p of image b (match[b,p] = m >= 0), l = decoded[b,p] and g = gt[b,m], both (x1, y1, x2, y2), L the
 * positive's term:   loss2[0] = alpha * sum of L over the positives of the batch;
 *                    d_raw_locs[b,p] = alpha * grad_scale * dL/dl;   (0,0,0,0) for every other prior.
 * MBX_LOC_L2: L = 1/2 |l - g|^2 -- loss2, d_raw_locs, d_logits and n_neg are byte-identical to mbx_loss_fwd_bwd_focal on
 * the same remaining arguments (the same float32 lines, the same reduction order).
 * Every other type is computed in float64: l and g are widened on load, L is accumulated in double, and alpha * grad_scale *
 * dL/dl is formed in double and rounded to float32 once.
 * MBX_LOC_SMOOTH_L1: L = sum over the four coordinates of s(|l_k - g_k|), s(d) = d^2 / (2 beta) if d < beta, else
 *   d - beta / 2 (d == beta is linear); the derivative is (l_k - g_k) / beta or its sign.  beta = loc_beta.
 * The IoU family first puts the PREDICTION in order (GIoU paper, Algorithm 2): X1 = min(l.x1, l.x2), X2 = max(l.x1, l.x2),
 * likewise Y1, Y2; the ground-truth box is taken as given (x1 <= x2, y1 <= y2 is the caller's to keep: with such boxes every
 * output is finite for finite inputs, points, zero-width and zero-area boxes included).  eps = 1e-7 and
 *   w = X2 - X1, h = Y2 - Y1, gw = g.x2 - g.x1, gh = g.y2 - g.y1
 *   iw = max(0, min(X2, g.x2) - max(X1, g.x1)), ih likewise, I = iw ih;   U = w h + gw gh - I;   IoU = I / (U + eps)
 *   cw = max(X2, g.x2) - min(X1, g.x1), ch likewise (the enclosing box)
 * MBX_LOC_GIOU: L = 1 - IoU + (cw ch - U) / (cw ch + eps)
 * MBX_LOC_DIOU: L = 1 - IoU + rho2 / (cw^2 + ch^2 + eps), rho2 = ((X1 + X2 - g.x1 - g.x2)^2 + (Y1 + Y2 - g.y1 - g.y2)^2) / 4
 * MBX_LOC_CIOU: L = DIoU's + a v, v = (4 / pi^2) (atan2(gw, gh) - atan2(w, h))^2, a = v / (1 - IoU + v + eps) held constant
 *   in the gradient (as in the CIoU paper); d atan2(w, h) = (h dw - w dh) / (w^2 + h^2), 0 where w^2 + h^2 == 0.
 * Kinks: a min or max takes its first argument at a tie, as written above, and its gradient goes there (so X1's goes to l.x1
 * when l.x1 <= l.x2, X2's to l.x1 when l.x1 >= l.x2); max(0, .) passes gradient only where its argument is > 0.
 * mbx_match's cost stays the reference's L2-based one whatever loc_type is; the location term reads the same `match`, so
 * threshold matching, mining and the focal term compose unchanged.  `alpha` (LOCATION_LOSS_ALPHA, 1000 in the reference)
 * was sized for L2 on corner residuals: a caller of the IoU types, whose L is of order 1 per positive, sets its own.
 * An unknown loc_type, a loc_beta that is not finite and > 0 with MBX_LOC_SMOOTH_L1 (it is ignored otherwise), or anything
 * mbx_loss_fwd_bwd_focal rejects: MBX_ERR_INVALID_ARG; workspace_bytes < mbx_loss_loc_workspace_bytes(B, P):
 * MBX_ERR_WORKSPACE (a bad argument is reported first); nothing is launched or written either way.  Two launches on
 * `stream`, one workgroup per image, graph-capturable, the same bytes on every call.
 * What any of these location terms does to AP on real data is NOT measured here: no trained model or dataset is at hand. */
enum { MBX_LOC_L2 = 0, MBX_LOC_SMOOTH_L1 = 1, MBX_LOC_GIOU = 2, MBX_LOC_DIOU = 3, MBX_LOC_CIOU = 4 };
size_t mbx_loss_loc_workspace_bytes(int B, int P);
int mbx_loss_fwd_bwd_loc(const float* decoded /*[B,P,4]*/, const float* conf_in /*[B,P]*/,
                         int conf_is_logit, const float* gt /*[B,G,4]*/,
                         const int32_t* match /*[B,P]*/, float alpha, float grad_scale, int B, int P,
                         int G, float* loss2 /*[2]*/,
                         float* d_raw_locs /*[B,P,4] or NULL*/, float* d_logits /*[B,P] or NULL*/,
                         int loc_type /*MBX_LOC_*/, float loc_beta /*MBX_LOC_SMOOTH_L1 only*/,
                         float gamma, float w_pos, float w_neg,
                         int neg_per_pos /*0 = every negative counts*/, int min_neg, int32_t* n_neg /*[B] or NULL*/,
                         void* workspace, size_t workspace_bytes, mbx_stream_t stream);

/* mbx_loss_fwd_bwd_loc with an IOU-AWARE CONFIDENCE TARGET (optional, not in the reference, off unless the caller asks): a
 * positive trains its confidence towards q, the IoU of its prediction with its box, not towards 1 -- the Quality Focal Loss
 * (Li et al. 2020, "Generalized Focal Loss") or the Varifocal Loss (Zhang et al. 2021, "VarifocalNet").  The one entry for
 * every combination of location term, mining and confidence term.  Every argument but `quality` and `q_stats` is
 * mbx_loss_fwd_bwd_loc's, same order and meaning.
 * MBX_QUALITY_NONE: loss2, d_raw_locs, d_logits and n_neg are byte-identical to mbx_loss_fwd_bwd_loc on the same remaining
 * arguments (the same launches); q_stats must be NULL.
 * MBX_QUALITY_QFL / MBX_QUALITY_VFL.  Per prior, s, c, w and ds are mbx_loss_fwd_bwd_focal's float32 quantities:
 *   s = sigmoid(conf_in) when conf_is_logit, else conf_in;   c = s + 1e-10f;   w = (1 - c) + 1e-10f
 *   ds = s (1 - s) when conf_is_logit, else 1
 * A negative keeps mbx_loss_fwd_bwd_focal's float32 lines: counted as there (every negative when neg_per_pos == 0, else the
 * selection of mbx_loss_fwd_bwd_mined -- the term is increasing in c, so the highest score is still the highest loss), its
 * term is -w_neg * c^gamma * log w, an unselected one adds nothing and gets +0.0f.
 * A positive (match[b,p] = m >= 0) is computed in float64 from the widened float32 values, l = decoded[b,p], g = gt[b,m]:
 *   q = IoU = I / (U + 1e-7) exactly as mbx_loss_fwd_bwd_loc's IoU family defines it: the prediction put in order first, the
 *     ground truth as given.  q is a CONSTANT in the gradient -- a target; nothing flows to d_raw_locs through it.
 *   t = q log c + (1 - q) log w                      dt/ds = q / c - (1 - q) / w
 *   QFL: M = |q - s|^gamma;  dM/ds = -gamma |q - s|^(gamma-1) sgn(q - s), exactly 0 where q == s (the kink passes no gradient,
 *        as max(0, .) in the location terms); with gamma == 0 M is the constant 1 and the dM term is left out.
 *   VFL: M = q;  dM/ds = 0.
 *   term L = -w_pos M t      dL/ds = -w_pos (dM/ds t + M dt/ds)      d_logits = (float)(dL/ds * ds * grad_scale), one rounding
 *   L goes into the image's confidence sum in double.  loss2[1] is the sum of all terms; nothing is normalised by the number
 *   of positives.  The papers' settings are w_pos = 1 with w_neg = 1 (QFL) or 0.75 (VFL), gamma = 2.
 * gamma is in [0, 10] as for the focal loss, and under QFL 0 or >= 1: for 0 < gamma < 1 the factor |q - s|^(gamma-1) is
 * unbounded as s -> q and a float32 gradient can overflow, so that range is refused.  At gamma == 1 the QFL gradient jumps
 * at q == s.  With c, w >= 1e-10 every term and gradient is finite for finite inputs: s exactly 0 or 1, q == 0 (disjoint
 * boxes) and degenerate predictions (inverted, zero-width, zero-area) included.
 * A VFL positive with q == 0 contributes neither loss nor gradient (the paper's behaviour; common in the first steps of
 * training).  A QFL positive with q == 0 is pushed down like a negative.
 * The location side (loss2[0], d_raw_locs), n_neg and the d_logits of every negative are byte-identical to
 * mbx_loss_fwd_bwd_loc with the same loc_type, loc_beta, gamma, w_neg, neg_per_pos and min_neg.
 * q_stats (may be NULL): q_stats[b] = {the sum of q over the positives of image b, their number}, both doubles, summed in a
 * fixed lane / wavefront order.  An image's outputs depend on its own row only, and the same input gives the same bytes on
 * every call (no floating-point atomics).  Any P.
 * An unknown quality, 0 < gamma < 1 with MBX_QUALITY_QFL, a q_stats with MBX_QUALITY_NONE, or anything mbx_loss_fwd_bwd_loc
 * rejects: MBX_ERR_INVALID_ARG; workspace_bytes < mbx_loss_quality_workspace_bytes(B, P): MBX_ERR_WORKSPACE (a bad argument
 * is reported first); nothing is launched or written either way.  Two launches on `stream`, one workgroup per image,
 * graph-capturable.
 * What either target does to AP on real data is NOT measured here: no trained model or dataset is at hand.             */
enum { MBX_QUALITY_NONE = 0, MBX_QUALITY_QFL = 1, MBX_QUALITY_VFL = 2 };
size_t mbx_loss_quality_workspace_bytes(int B, int P);
int mbx_loss_fwd_bwd_quality(const float* decoded /*[B,P,4]*/, const float* conf_in /*[B,P]*/,
                             int conf_is_logit, const float* gt /*[B,G,4]*/,
                             const int32_t* match /*[B,P]*/, float alpha, float grad_scale, int B, int P,
                             int G, float* loss2 /*[2]*/,
                             float* d_raw_locs /*[B,P,4] or NULL*/, float* d_logits /*[B,P] or NULL*/,
                             int loc_type /*MBX_LOC_*/, float loc_beta /*MBX_LOC_SMOOTH_L1 only*/,
                             int quality /*MBX_QUALITY_*/, float gamma, float w_pos, float w_neg,
                             int neg_per_pos /*0 = every negative counts*/, int min_neg, int32_t* n_neg /*[B] or NULL*/,
                             double* q_stats /*[B,2] or NULL*/,
                             void* workspace, size_t workspace_bytes, mbx_stream_t stream);

/* mbx_loss_fwd_bwd_quality with the IGNORE BAND of mbx_match_ignore (optional, not in the reference, off unless the caller
 * asks): the one entry for every combination of location term, mining, confidence term and band.  Every argument is
 * mbx_loss_fwd_bwd_quality's, same order and meaning -- MBX_QUALITY_NONE with gamma == 0 and weights (1, 1) is the plain
 * confidence term, q_stats must be NULL with MBX_QUALITY_NONE -- and `match` has three states:
 *   match[b,p] >= 0: a positive of that box;
 *   match[b,p] == MBX_MATCH_IGNORED (-2): neither.  The prior adds nothing to loss2[0] or loss2[1]; its d_raw_locs are
 *     (0,0,0,0) and its d_logits is +0.0f whatever the sign of grad_scale; it is no candidate of the mining's select and no
 *     positive; it does not enter q_stats;
 *   any other negative value (-1, -3, -77, ...): a negative, as in the other entries.
 * With ign = the number of ignored priors of image b and n_pos its positives:  N_neg = P - n_pos - ign, and
 *   neg_per_pos == 0: every negative counts, n_neg[b] = N_neg;
 *   neg_per_pos >= 1: K = min(N_neg, max(min_neg, neg_per_pos * n_pos)), the first K of the negatives in
 *     mbx_loss_fwd_bwd_mined's order (the same key on conf_in, the index as the tie-break) are selected, n_neg[b] = K.
 * The outputs are those of mbx_loss_fwd_bwd_quality on the image with its ignored priors REMOVED (taking priors out keeps the
 * others' relative index order, so the selection is the same set): d_raw_locs and d_logits of every kept prior, n_neg and the
 * count in q_stats are byte-identical to that call; loss2 and the sum in q_stats are the same terms summed in another lane
 * order.  With no -2 in `match`, every output is byte-identical to mbx_loss_fwd_bwd_quality on the same arguments.
 * An image's outputs depend on its own row only, and the same input gives the same bytes on every call.  Any P.
 * Anything mbx_loss_fwd_bwd_quality rejects: MBX_ERR_INVALID_ARG; workspace_bytes < mbx_loss_ignore_workspace_bytes(B, P):
 * MBX_ERR_WORKSPACE (a bad argument is reported first); nothing is launched or written either way.  Two launches on
 * `stream`, one workgroup per image, graph-capturable.
 * What the band does to AP on real data is NOT measured here: no trained model or dataset is at hand.                  */
size_t mbx_loss_ignore_workspace_bytes(int B, int P);
int mbx_loss_fwd_bwd_ignore(const float* decoded /*[B,P,4]*/, const float* conf_in /*[B,P]*/,
                            int conf_is_logit, const float* gt /*[B,G,4]*/,
                            const int32_t* match /*[B,P]: >= 0, MBX_MATCH_IGNORED or another negative*/, float alpha,
                            float grad_scale, int B, int P, int G, float* loss2 /*[2]*/,
                            float* d_raw_locs /*[B,P,4] or NULL*/, float* d_logits /*[B,P] or NULL*/,
                            int loc_type /*MBX_LOC_*/, float loc_beta /*MBX_LOC_SMOOTH_L1 only*/,
                            int quality /*MBX_QUALITY_*/, float gamma, float w_pos, float w_neg,
                            int neg_per_pos /*0 = every negative counts*/, int min_neg, int32_t* n_neg /*[B] or NULL*/,
                            double* q_stats /*[B,2] or NULL*/,
                            void* workspace, size_t workspace_bytes, mbx_stream_t stream);

/* ------------------------------------------------- detect post-processing (A9-A12)
 * Replaces the per-patch numpy loop detect.py:408-436: decode + clip [0,1]
 * (412-413), filter_proposals (74-104, strict inequalities), sort by confidence
 * descending and keep max_to_keep (423-427), convert_proposals to image coordinates in
 * float64 incl. the flip (106-131).  Ties in confidence: higher prediction index first
 * (the reference's order among ties is undefined).  `conf` may hold ANY float (the sort key is an order-
 * preserving image of the float bits): negative values, values >= 1 and infinities order as numpy's
 * argsort does; a NaN sorts first, as argsort(...)[::-1] (detect.py:423) places it.
 * A NaN COORDINATE is clipped to 0 (fminf(fmaxf(x, 0), 1)) and filtered and reported as 0; numpy's clip keeps the NaN, which
 * then passes the reference's strict filter.  out_count[b] = clamp(min(kept, max_to_keep), 0, k_max); the slots at or past it
 * are 0.0 / 0.0f / -1.  P <= 16384, above: MBX_ERR_UNSUPPORTED, nothing launched or written.                          */
typedef struct {
  int32_t offset_y, offset_x; /* batched_offsets  (detect.py:190-281) */
  int32_t patch_h, patch_w;   /* batched_dims */
  int32_t image_h, image_w;   /* batched_heights_widths */
  int32_t is_flipped;
  int32_t max_to_keep;
  float restrictions[4];      /* x1,y1,x2,y2 (detect.py:50-54) */
} mbx_patch_meta;

int mbx_decode_filter_topk(const float* raw_locs /*[B,P,4]*/, const float* conf /*[B,P]*/,
                           const float* priors /*[P,4]*/, const mbx_patch_meta* meta /*[B]*/,
                           int B, int P, int k_max, double* out_boxes /*[B,k_max,4]*/,
                           float* out_scores /*[B,k_max]*/, int32_t* out_index /*[B,k_max]*/,
                           int32_t* out_count /*[B]*/, mbx_stream_t stream);

/* OPTIONAL greedy non-maximum suppression per patch on the output of mbx_decode_filter_topk, in place (row N1: BASELINE's
 * north_star names an NMS stage; the reference has none -- detect.py:408-443 keeps the top max_to_keep boxes -- so it is
 * off by default and outside the parity path).  Boxes are taken in their stored (score-descending) order; box i is
 * dropped iff IoU(i, j) > iou_threshold for an earlier KEPT box j; survivors are compacted to the front of each row of
 * out_boxes / out_scores / out_index and out_count[b] becomes their number.  IoU in float64, k_max <= 1024 (above:
 * MBX_ERR_UNSUPPORTED, nothing launched or written).  count[b] is clamped to [0, k_max] on the way in; the slots at or
 * past the new count keep what they held.                                                                             */
int mbx_nms(double* boxes /*[B,k_max,4] x1,y1,x2,y2*/, float* scores /*[B,k_max]*/, int32_t* index /*[B,k_max]*/,
            int32_t* count /*[B], in/out*/, int B, int k_max, double iou_threshold, mbx_stream_t stream);

/* OPTIONAL per-image merge of multi-crop detections (not in the reference, which writes every patch's boxes one after the
 * other -- detect.py:438-460 -- so an object is reported once per patch that sees it).  Input: exactly what
 * mbx_decode_filter_topk (+ mbx_nms) writes, rows in stream order; image i owns rows [image_rows[i], image_rows[i+1]).
 * Per image: the candidates are the slots [0, count[r]) of its rows (count clamped to [0, k_max]; a row need not be
 * sorted), flat index row * k_max + slot.  They are ordered by score descending, ties by ascending flat index (the same
 * order-preserving image of the float bits as mbx_decode_filter_topk: -0 == +0, a NaN first), and walked greedily: a
 * candidate is kept iff its IoU with every earlier KEPT candidate is <= iou_threshold (float64, the operation order of
 * mbx_nms; +infinity = no suppression, no IoU is evaluated), until max_det are kept or the list ends.  Kept candidates go
 * out in kept order: out_boxes (the source's bytes), out_scores, out_src (flat index), out_count[i]; unused slots are
 * 0 / 0 / -1.  out_status[i]: 0 ok; 1 = more than MBX_MERGE_MAX_CANDIDATES candidates, out_count[i] = 0 (the caller cuts
 * such an image down first).  I == 0: MBX_OK, nothing launched.  max_det <= 640 (what the kernel's LDS holds beside the
 * 16 384 sort keys), above: MBX_ERR_UNSUPPORTED.  Not in place, one workgroup per image.                            */
#define MBX_MERGE_MAX_CANDIDATES 16384
int mbx_merge_detections(const double* boxes /*[R,k_max,4] x1,y1,x2,y2*/, const float* scores /*[R,k_max]*/,
                         const int32_t* count /*[R]*/, const int32_t* image_rows /*[I+1] ascending*/, int I, int k_max,
                         int max_det, double iou_threshold, double* out_boxes /*[I,max_det,4]*/,
                         float* out_scores /*[I,max_det]*/, int32_t* out_src /*[I,max_det]*/,
                         int32_t* out_count /*[I]*/, int32_t* out_status /*[I]*/, mbx_stream_t stream);

/* mbx_merge_detections with BOX VOTING (optional, off by default in detect.py): every kept box is replaced by the
 * score-weighted mean of all candidates of its image that overlap it strongly.  The kept list, its order, out_scores,
 * out_src, out_count and out_status are exactly what mbx_merge_detections writes for the same arguments (the same kernel
 * runs first): iou_threshold = +infinity (plain top-N), the max_det cut and the status-1 refusal above
 * MBX_MERGE_MAX_CANDIDATES included.  The candidates of image i are the slots [0, clamp(count[r], 0, k_max)) of its rows,
 * as above -- EVERY one: suppressed ones, kept ones and the ones past the max_det cut; a slot at or past count[r] is
 * never read.  Candidate c VOTES for kept box e iff its score is finite and > 0 (a NaN, +-0, a negative score and
 * +infinity do not vote) and IoU(e, c) >= vote_iou_threshold, the IoU in float64 in the operation order of mbx_nms
 * (iw = min(e.x2, c.x2) - max(e.x1, c.x1), ih alike; inter = iw > 0 && ih > 0 ? iw * ih : 0; uni = area(e) + area(c) -
 * inter; uni > 0 ? inter / uni : 0), so membership is exact against a numpy restatement.  A kept box of positive width
 * and height with a votable score votes for itself (IoU exactly 1); a kept box of area <= 0 has no voters.
 *   out_votes[i,k]  the number n of voters; unused slots 0
 *   out_boxes[i,k]  n == 0: the kept candidate's own bytes, as in the plain merge; otherwise coordinate j is
 *                   (sum_c w_c * x_cj) / (sum_c w_c) in float64 with w_c = (double)score_c, every product rounded once
 *                   (no fused multiply-add); unused slots 0
 * The sums are taken in an order that is a function of the image's own rows only (per lane over the rows in order, then
 * a fixed tree; no floating-point atomics): an image's outputs do not depend on I, on its place in the launch or on the
 * other images, and the same input gives the same bits on every call.  Any order keeps
 * |out - exact| <= (2n + 4) * 2^-53 * (sum w|x|) / (sum w) per coordinate.
 * vote_iou_threshold outside (0, 1] or NaN, or a null out_votes: MBX_ERR_INVALID_ARG, nothing launched; every other check
 * as mbx_merge_detections (max_det > 640: MBX_ERR_UNSUPPORTED; I == 0: MBX_OK, nothing launched).  Two launches on
 * `stream`: the merge (one workgroup per image), then the vote (one wavefront per two kept boxes).
 * Whether voting raises AP on real data is NOT measured here: no trained model or dataset is at hand.             */
int mbx_merge_detections_voted(const double* boxes /*[R,k_max,4] x1,y1,x2,y2*/, const float* scores /*[R,k_max]*/,
                               const int32_t* count /*[R]*/, const int32_t* image_rows /*[I+1] ascending*/, int I,
                               int k_max, int max_det, double iou_threshold, double vote_iou_threshold,
                               double* out_boxes /*[I,max_det,4]*/, float* out_scores /*[I,max_det]*/,
                               int32_t* out_src /*[I,max_det]*/, int32_t* out_count /*[I]*/,
                               int32_t* out_status /*[I]*/, int32_t* out_votes /*[I,max_det]*/, mbx_stream_t stream);

/* SOFT-NMS in the per-image merge (Bodla et al. 2017; optional, off by default in detect.py): instead of deleting a
 * candidate that overlaps a picked box, lower its score by a function of the IoU and let it compete again.  Inputs, the
 * candidate set (slots [0, clamp(count[r], 0, k_max)) of the image's rows, flat index row * k_max + slot), out_status
 * (1 above MBX_MERGE_MAX_CANDIDATES, out_count[i] = 0) and the unused output slots (0 / 0 / -1) are those of
 * mbx_merge_detections.  Per image:
 *   1. every candidate c has a working score t_c = (double)score_c.
 *   2. c is LIVE iff t_c is finite and t_c > min_score.  A NaN, +-infinity and everything at or below min_score never
 *      take part: they are not picked and decay nobody.  Weights are <= 1, so a candidate that leaves the live set never
 *      returns.
 *   3. repeat while fewer than max_det are picked and a live candidate exists:
 *        PICK   the live candidate p with the largest t, bit-equal t resolved by ascending flat index.  The next output
 *               slot gets p's box bytes, (float)t_p (round to nearest) and p's flat index.  p leaves the live set.
 *        DECAY  for every live c: o = IoU(p, c) -- the float64 IoU of mbx_nms, term by term, with p as the EARLIER box
 *               (iw = min(p.x2, c.x2) - max(p.x1, c.x1), ih alike; inter = iw > 0 && ih > 0 ? iw * ih : 0;
 *               uni = area(p) + area(c) - inter; o = uni > 0 ? inter / uni : 0) -- then t_c = t_c * w, ONE rounded
 *               multiply, with
 *                 MBX_SOFT_LINEAR    w = o > iou_threshold ? 1.0 - o : 1.0
 *                 MBX_SOFT_GAUSSIAN  w = exp(-(o * o) / sigma): one rounded product, one rounded division, a negation,
 *                                    then exp (the device's float64 exp, documented to 1 ulp).  o == 0 gives exactly 1.
 *               No fused multiply-add anywhere.
 *   4. out_count[i] = the number of picks.  Picks come out in pick order; scores only fall, so out_scores is
 *      non-increasing and the first max_det picks are exactly the max_det best of an uncut Soft-NMS.
 * Linear: every operation is a single rounded float64 operation in a stated order, so all outputs are exact against a
 * numpy restatement.  Gaussian: exact but for exp.
 * vote_iou_threshold in (0, 1]: the vote launch of mbx_merge_detections_voted follows on the same stream -- its contract,
 * out_votes and error bound unchanged; the voters' weights are the ORIGINAL scores, the kept boxes the picks.  0: no
 * voting, out_votes is not touched (NULL iff vote_iou_threshold == 0).
 * An image's outputs depend on its own rows only -- not on I, its place in the launch or the other images -- and the same
 * input gives the same bytes on every call: each t_c is a product over the picks in pick order, whichever thread owns c.
 * MBX_ERR_INVALID_ARG, nothing launched: a method other than 1 or 2; linear with a NaN iou_threshold; gaussian with sigma
 * not finite or <= 0; min_score NaN, negative or infinite; vote_iou_threshold NaN or outside [0, 1]; vote_iou_threshold > 0
 * with a null out_votes; any null pointer the plain merge rejects, I < 0, k_max <= 0, max_det <= 0.  max_det > 640:
 * MBX_ERR_UNSUPPORTED, as for the other two entry points.  I == 0: MBX_OK, nothing launched.  iou_threshold is read by the
 * linear method only, sigma by the gaussian only.  One workgroup per image; every pick is a pass over the image's live
 * candidates.  Whether Soft-NMS raises AP on real data is NOT measured here: no trained model or dataset is at hand.  */
#define MBX_SOFT_LINEAR 1
#define MBX_SOFT_GAUSSIAN 2
int mbx_merge_detections_soft(const double* boxes /*[R,k_max,4] x1,y1,x2,y2*/, const float* scores /*[R,k_max]*/,
                              const int32_t* count /*[R]*/, const int32_t* image_rows /*[I+1] ascending*/, int I, int k_max,
                              int max_det, int method, double iou_threshold /*linear only*/, double sigma /*gaussian only*/,
                              double min_score, double vote_iou_threshold /*0 = no voting*/,
                              double* out_boxes /*[I,max_det,4]*/, float* out_scores /*[I,max_det]*/,
                              int32_t* out_src /*[I,max_det]*/, int32_t* out_count /*[I]*/, int32_t* out_status /*[I]*/,
                              int32_t* out_votes /*[I,max_det]; NULL iff vote_iou_threshold == 0*/, mbx_stream_t stream);

/* WEIGHTED BOXES FUSION in the per-image merge (Solovyev, Wang, Gabruseva 2021; optional, off by default in detect.py):
 * the three entry points above select among an image's candidates; this one clusters them against the running fused box
 * of each cluster, reports the clusters, and scores a cluster by how many candidates agree on it.  The inputs, the
 * candidate set (slots [0, clamp(count[r], 0, k_max)) of the image's rows), the flat index row * k_max + slot,
 * out_status 1 with out_count 0 above MBX_MERGE_MAX_CANDIDATES, I == 0 (MBX_OK, nothing launched) and max_det > 640
 * (MBX_ERR_UNSUPPORTED) are those of mbx_merge_detections.  R is the number of rows of boxes / scores / count; an image
 * whose rows are not within [0, R] gets out_status 2 and out_count 0, and nothing of it is read.  Per image:
 *   1. t_c = (double)score_c.  A candidate is LIVE iff t_c is finite and t_c > min_score.  Everything else (NaN, +-inf, 0,
 *      negatives, anything at or below min_score) takes no part anywhere.
 *   2. the live candidates are walked by score descending, ties by ascending flat index (the order of the plain merge).
 *   3. clusters are numbered in creation order.  For candidate c with box x, area a = (x2 - x1) * (y2 - y1), weight t:
 *      against every existing cluster k, o_k = IoU(F_k, x) -- the float64 IoU of mbx_nms, term by term, with the fused
 *      box as the EARLIER box and the stored areas A_k and a (iw = min(F.x2, x.x2) - max(F.x1, x.x1), ih alike;
 *      inter = iw > 0 && ih > 0 ? iw * ih : 0; uni = A_k + a - inter; o = uni > 0 ? inter / uni : 0).  m = the cluster
 *      with the largest o_k, bit-equal values to the lowest k.
 *        o_m > iou_threshold (strict): c JOINS m.  S_m += t; X_mj += t * x_j for j = 0..3 (the product rounded once,
 *               then the sum; no fused multiply-add); n_m += 1; F_mj = X_mj / S_m; A_m = (F_m2 - F_m0) * (F_m3 - F_m1).
 *        otherwise c FOUNDS a cluster: S = t, X_j = t * x_j, n = 1, F = x's own bytes, A = a, first = c's flat index.
 *   4. the cluster's score in float64: q = S / (double)n (MBX_WBF_AVG) or the t of its first member (MBX_WBF_MAX); if
 *      expected_views > 1, q = (q * (double)min(n, expected_views)) / (double)expected_views.  out_scores = (float)q.
 *   5. clusters go out by the order image of that float32 score, descending, ties by ascending cluster number, cut to
 *      max_det: out_boxes = F (a cluster with n == 1 therefore carries its candidate's own bytes), out_src = first,
 *      out_votes = n, out_count = min(clusters, max_det).  Unused slots 0 / 0 / -1 / 0.
 * Every operation is one rounded float64 operation in a stated order and the walk is sequential, so all outputs are exact
 * against a numpy restatement; they depend on the image's own rows only -- not on I, its place in the launch or the
 * other images -- and the same input gives the same bytes on every call.  iou_threshold = 1 never joins anything: for
 * inputs whose scores are all live the outputs then equal mbx_merge_detections with iou_threshold = +infinity.
 * workspace: mbx_merge_wbf_workspace(R, k_max) bytes of device memory, 8-byte aligned, contents irrelevant before and
 * after the call (host only; 0 for sizes it refuses: R <= 0, k_max <= 0, R * k_max >= 2^31).
 * MBX_ERR_INVALID_ARG, nothing launched: conf_type not 1 or 2; iou_threshold NaN or outside [0, 1]; min_score NaN,
 * negative or infinite; expected_views < 1; a null out_votes or workspace; workspace_bytes below what
 * mbx_merge_wbf_workspace returns (or a size it refuses); everything the plain merge rejects.  One workgroup per image,
 * one launch; every live candidate is a sequential step with a pass over the image's clusters.  Whether fusion raises AP
 * on real data is NOT measured here: no trained model or dataset is at hand.                                          */
#define MBX_WBF_AVG 1
#define MBX_WBF_MAX 2
size_t mbx_merge_wbf_workspace(int R, int k_max);
int mbx_merge_detections_wbf(const double* boxes /*[R,k_max,4] x1,y1,x2,y2*/, const float* scores /*[R,k_max]*/,
                             const int32_t* count /*[R]*/, const int32_t* image_rows /*[I+1] ascending*/, int R, int I,
                             int k_max, int max_det, int conf_type, double iou_threshold, double min_score,
                             int expected_views, double* out_boxes /*[I,max_det,4]*/, float* out_scores /*[I,max_det]*/,
                             int32_t* out_src /*[I,max_det]*/, int32_t* out_count /*[I]*/, int32_t* out_status /*[I]*/,
                             int32_t* out_votes /*[I,max_det]*/, void* workspace, size_t workspace_bytes,
                             mbx_stream_t stream);

/* ------------------------------------------------------ COCO metric: matching (eval.py:212-226)
 * Replaces the matching step of the metric eval.py:212-226 runs: pycocotools' COCOeval.evaluateImg (iouType 'bbox',
 * useCats = 0, no crowd annotations), once per image, area range and IoU threshold; multibox_amd/cocoeval.py:_evaluate_img
 * restates it and is the definition.  Image i owns detections [dt_rows[i], dt_rows[i+1]) -- ALREADY in evaluation order
 * (score descending, stable) and cut to MBX_COCO_MAX_DET -- and gts [gt_rows[i], gt_rows[i+1]) in annotation order.
 * Per (image, range [a0, a1], threshold t): the gts are taken with the in-range ones (a0 <= area <= a1, the annotation's
 * area column) first, stably; each detection in order takes, among the gts no earlier detection took, the in-range one
 * with the largest IoU >= min(t, 1 - 1e-10), of equal IoUs the later; only if there is none, the same among the
 * out-of-range ones.  IoU in float64 in the operation order of cocoeval._iou_xywh (x1 = x + w; iw = max(min - max, 0);
 * union = (dw*dh + gw*gh) - inter; union > 0 ? inter / union : 0), so every comparison is the host's.  iou_thrs and
 * area_rng are HOST arrays, read before the call returns (pass cocoeval.IOU_THRS: np.linspace's values are part of the
 * parity).  All inputs must be finite.
 *   match[i,a,t,d]   the gt's row within its image in ANNOTATION order, or -1
 *   ignore[i,a,t,d]  1 iff the matched gt is out of range, or d is unmatched and its own area w*h is < a0 or > a1
 *   n_gt_counted[i,a] number of in-range gts
 *   slots d past the image's detections: -1 / 0
 *   status[i]        0 ok; 1 = more than MBX_COCO_MAX_GT gts or MBX_COCO_MAX_DET detections: outputs -1 / 0 / 0, the
 *                    caller computes that image on the host
 * I == 0: MBX_OK, nothing launched.  T outside [1,16] or A outside [1,8]: MBX_ERR_INVALID_ARG.  One workgroup per image,
 * one wavefront per threshold.                                                                                        */
#define MBX_COCO_MAX_DET 100
#define MBX_COCO_MAX_GT 128
int mbx_coco_match(const double* dt /*[ND,5] x,y,w,h,score*/, const int32_t* dt_rows /*[I+1] ascending*/,
                   const double* gt /*[NG,5] x,y,w,h,area*/, const int32_t* gt_rows /*[I+1] ascending*/, int I,
                   const double* iou_thrs /*HOST [T], T <= 16*/, int T, const double* area_rng /*HOST [A,2], A <= 8*/,
                   int A, int16_t* match /*[I,A,T,MBX_COCO_MAX_DET]*/, uint8_t* ignore /*[I,A,T,MBX_COCO_MAX_DET]*/,
                   int32_t* n_gt_counted /*[I,A]*/, int32_t* status /*[I]*/, mbx_stream_t stream);

/* ------------------------------------------------------ COCO metric: accumulation (eval.py:227-246)
 * Replaces the accumulation step of the same metric: pycocotools' COCOeval.accumulate for one category, on the outputs of
 * mbx_coco_match; multibox_amd/cocoeval.py:accumulate_tables restates it and is the definition.  dt and dt_rows are the
 * ones given to mbx_coco_match, under the same PRECONDITION: per image the detections are by score descending, stable,
 * cut to MBX_COCO_MAX_DET (so an image's slot k never sorts before its slot k-1, and the first detection of the global
 * order has slot 0).  match / ignore / n_gt_counted are what mbx_coco_match wrote (a refused image's rows filled in by the
 * caller); of match only `>= 0` is read, of ignore only `!= 0`.  ND = dt_rows[I] is read from the device before anything
 * is launched (one 4-byte copy and a wait on `stream`): the grids depend on it.
 * The detections are ordered by score descending, ties by ascending row of dt (-0.0 == +0.0), which is
 * argsort(-score, kind="mergesort").  For maxDets value max_dets[m] a detection takes part iff its slot within its image
 * is < max_dets[m].  Per slice (t, a, m), over the detections that take part, in that order, with
 * npig = sum_i n_gt_counted[i,a]:
 *   tp[k] = number of k' <= k with match >= 0 and not ignore      fp[k] = ... with match < 0 and not ignore
 *   rc[k] = tp[k] / npig      pr[k] = max over k' >= k of tp[k'] / ((fp[k'] + tp[k']) + 2.220446049250313e-16)
 *   precision[t,r,a,m] = pr at the first k with rc[k] >= rec_thrs[r], 0 if there is none
 *   recall[t,a,m]      = rc at the last k, 0 if no detection takes part
 * in float64 in exactly this operation order, so the values are the host's bit for bit.  npig == 0: the slice's entries
 * are -1.  rec_thrs and max_dets are HOST arrays, read before the call returns (pass cocoeval.REC_THRS: np.linspace's
 * values are part of the parity).  I == 0: MBX_OK, both tables -1, nothing else launched.
 * Limits: T in [1,16], A in [1,8] (mbx_coco_match's), R in [1,MBX_COCO_ACC_MAX_R], M in [1,MBX_COCO_ACC_MAX_M], a null
 * pointer or workspace_bytes < mbx_coco_accumulate_workspace(ND, T, A, M): MBX_ERR_INVALID_ARG.  ND >
 * MBX_COCO_ACC_MAX_ND: MBX_ERR_UNSUPPORTED.  Either way nothing is written and no detection is read.
 * Workspace (no state survives a call; 256-byte aligned): with W = ceil(T A / 32) and S = T A M,
 * ND (24 + 8 W + 1) bytes for the sort's two (key, index) buffers and the gathered flag bits, plus
 * 16 S (ceil(ND / MBX_COCO_ACC_CHUNK) + 1) bytes of per-chunk totals and maxima, plus rounding: at most 89 bytes per
 * detection (T = 16, A = 8, M = 4), 48.5 for COCO's 10 / 4 / 3.  mbx_coco_accumulate_workspace is host-only and returns
 * 0 for sizes outside the limits.  Separate launches on `stream` (tile sort of MBX_COCO_ACC_SORT_TILE elements, merge
 * passes, gather, chunk totals, their scan, chunk maxima, their suffix maximum, search); no workgroup waits on another. */
#define MBX_COCO_ACC_MAX_R 128
#define MBX_COCO_ACC_MAX_M 4
#define MBX_COCO_ACC_MAX_ND 4194304
#define MBX_COCO_ACC_CHUNK 256
#define MBX_COCO_ACC_SORT_TILE 1024
size_t mbx_coco_accumulate_workspace(long long ND, int T, int A, int M);
int mbx_coco_accumulate(const double* dt /*[ND,5] x,y,w,h,score*/, const int32_t* dt_rows /*[I+1] ascending*/, int I,
                        const int16_t* match /*[I,A,T,MBX_COCO_MAX_DET]*/, const uint8_t* ignore /*[I,A,T,MBX_COCO_MAX_DET]*/,
                        const int32_t* n_gt_counted /*[I,A]*/, int T, int A, const double* rec_thrs /*HOST [R]*/, int R,
                        const int32_t* max_dets /*HOST [M]*/, int M, double* precision /*[T,R,A,M]*/,
                        double* recall /*[T,A,M]*/, void* workspace, size_t workspace_bytes, mbx_stream_t stream);

/* ------------------------------------------------------------ convolution stack (A2-A4)
 * Replaces slim.conv2d (+ batch_norm + relu) of model.py:6-324 and its TF gradients
 * (train.py:263).  Activations are NHWC bf16 *views*: element (n,h,w,c) of a tensor lives at
 * base[n*img_stride + (h*W + w)*ld + c], so a branch can read/write a channel slice of a
 * wider concat buffer (tf.concat(3, ...) of model.py:18,38,58,138,159,182 costs nothing).
 * Filters are bf16 [C_out][R][S][C_in] (KRSC), contiguous.  Accumulation is fp32 on MFMA
 * (v_mfma_f32_16x16x32_bf16).  C_in, ld and slice offsets must be multiples of 8.
 *
 * mbx_conv_desc.transposed = 1 computes the data gradient: the same kernel run on dy with
 * the spatially flipped, channel-transposed filter ([C_in][R][S][C_out], see
 * mbx_filter_prepare) and an input dilated by `stride`.                                 */
typedef enum {
  MBX_EPI_STORE = 0,    /* y = acc [* rscale] [+ y if accumulate] [* (skip > 0): relu backward mask]
                           (bf16; pre-BN activations, gradients)                           */
  MBX_EPI_AFFINE = 1,   /* y = act(acc*scale[c] + shift[c])       (frozen / folded batch norm) */
  MBX_EPI_RESIDUAL = 2, /* y = act(skip + rscale*(acc + shift[c]))           (model.py:19-23) */
  MBX_EPI_STORE_F32 = 3 /* y = acc as float32            (head outputs, model.py:213-293)     */
} mbx_epilogue;

/* BATCH-NORM BACKWARD STATISTICS FROM THE DATA GRADIENT THAT WRITES THE ACTIVATION GRADIENT (round 4).  The backward pass of
 * slim.batch_norm + relu (train.py:94-99) needs, per channel, sum g and sum g xhat over all pixels before it can write one
 * element -- with g = da (a > 0): a grid-wide dependency that cost a grid barrier per layer (mbx_bn_bwd_onepass) or three
 * launches.  The convolution whose data gradient WRITES da already holds every element of it in registers: with this table
 * attached to its descriptor (mbx_conv_desc.bn_bwd_stats) its epilogue also reads y at the same positions and ADDS
 *   sum g  and  sum g y,   g = (y > relu_thr[c]) ? bf16(da) : 0
 * (float32 atomics) into row (tile index mod rows_mod) of stats[i] = [rows_mod][stats_ld[i]][2], ZERO at launch.  Output
 * channels [c_begin[i], c_begin[i+1]) of the launch belong to entry i (at most 4: the gradient of a concat buffer slice
 * feeds several layers): y[i] = that layer's pre-BN output [M, ld_y[i]] at the entry's first channel, relu_thr[i] / stats[i]
 * likewise.  c_begin ascending from 0 in multiples of 32.  mbx_bn_bwd_apply_rows then is ONE streaming launch.
 * (sum g xhat = rstd (sum g y - mean sum g); the mask y > mean - beta / rstd is the forward's (y - mean) rstd + beta > 0.)
 * Plain bf16 STORE data gradients only (no accumulate, no mask, stride 1); anything else: MBX_ERR_INVALID_ARG / UNSUPPORTED. */
typedef struct {
  int32_t n, rows_mod;
  int32_t c_begin[4];
  const void* y[4]; int32_t ld_y[4];
  const float* relu_thr[4];
  float* stats[4]; int32_t stats_ld[4];
} mbx_bn_bwd_stats;

/* THE BATCH-NORM APPLY OF A TRAINING-MODE CONVOLUTION AS THE TAIL OF ITS OWN LAUNCH (round 6).  slim.conv2d in training mode
 * (train.py:94-105: convolution, batch statistics, normalise + beta, relu) was two launches: the convolution, adding its
 * tile sums into the fixed-point statistics rows (stats_rows_mod > 0), and mbx_bn_apply_fused_mapped.  With this table
 * attached (mbx_conv_desc.bn_apply) the convolution's workgroups, when their last tile is stored, meet at a ONE-SHOT GRID
 * BARRIER, reduce the rows of every channel themselves and normalise THE TILES THEY WROTE (read back from their own CU's L2):
 * one launch, the same mean / rstd / relu threshold / moving statistics / activations bit for bit.
 *   barrier: DEVICE, MBX_GRID_BARRIER_BYTES, 128-byte aligned, ZERO at launch, used by one launch per clearing.
 *   The launch takes at most one workgroup per CU (max_workgroups caps it further); if its workgroups are NOT co-resident
 *   (CUs held by another stream's kernels) the barrier times out: those workgroups write NaN activations and add 1 to
 *   *step_poison (word [0] of the step control block: the optimiser then skips the step on every rank) -- the caller falls
 *   back to the two-launch form.
 * Persistent / one-tile-per-workgroup launches only (tile_config 33..39, 97, 98), bf16 STORE with statistics, y rows
 * contiguous per image (y_img_stride = H_out W_out ldy), not a member of mbx_conv_pair; anything else: MBX_ERR_UNSUPPORTED. */
#define MBX_GRID_BARRIER_BYTES 6400
typedef struct {
  void* barrier;
  void* a; int32_t ld_a;                /* activation: a[m * ld_a + c], m = img * H_out * W_out + pixel (bf16)      */
  const float* beta;                    /* [C_out]                                                                   */
  float* mean; float* rstd;             /* [C_out] out: batch mean, 1 / sqrt(var + eps)                              */
  float* moving_mean; float* moving_var;/* may be NULL; decay < 0: STORE mode (batch mean / biased variance), else
                                           moving -= (1 - decay) (moving - batch)                                    */
  float* relu_thr;                      /* may be NULL: mean - beta / rstd (relu) or -inf                            */
  int32_t relu; float eps, decay;
  float* step_poison;                   /* may be NULL                                                               */
} mbx_bn_apply_desc;

/* THE BATCH-NORM BACKWARD OF THE LAYERS A DATA GRADIENT FEEDS, AS THE TAIL OF THAT DATA-GRADIENT LAUNCH (round 6).  The
 * convolution whose data gradient WRITES the activation gradient da of batch-norm layers (train.py:94-99 on the way back,
 * train.py:263) finishes their backward itself: when a workgroup's last tile is stored it sweeps THE TILES IT WROTE (da back
 * from its own CU's L2, y from memory) for its share of  sum g  and  sum g xhat  (g = da where the activation was positive:
 * xhat + beta > 0 recomputed from y), adds them into the layers' accumulators (float atomics), meets the other workgroups at
 * a ONE-SHOT GRID BARRIER, reads the totals and sweeps its tiles again to write
 *   dy = rstd (g - mean g - xhat mean g xhat),   dbeta += sum g
 * -- what mbx_bn_bwd_onepass computed in a launch of its own.  Output channels [c_begin[i], c_begin[i+1]) of the launch belong
 * to entry i (at most 4: the gradient of a concat-buffer slice feeds several layers); y / dy / mean / rstd / beta / dbeta /
 * acc are that layer's, AT THE ENTRY'S FIRST CHANNEL; acc = [MBX_BN_BWD_SLOTS][2][acc_ld] float32, ZERO at launch; c_begin
 * ascending from 0 in multiples of 8; relu[i]: the layer has a relu behind its batch norm.  Every channel of da must be
 * written by this launch alone (plain bf16 STORE, no accumulate / mask / sign bits / statistics, stride 1, rows of da
 * contiguous per image).  barrier / step_poison / residency / time-out: as mbx_bn_apply_desc.  tile_config 33..39, 97, 98
 * only; anything else: MBX_ERR_UNSUPPORTED.  Same mathematics as mbx_bn_bwd_onepass; like it, the float atomics make the
 * last bits depend on the order of arrival.                                                                              */
#define MBX_BN_BWD_SLOTS 8
typedef struct {
  void* barrier;
  int32_t n;
  int32_t c_begin[4];
  const void* y[4]; int32_t ld_y[4];
  void* dy[4]; int32_t ld_dy[4];
  const float* mean[4]; const float* rstd[4]; const float* beta[4];
  float* dbeta[4];
  float* acc[4]; int32_t acc_ld[4];
  int32_t relu[4];
  float* step_poison;
} mbx_bn_bwd_fused;

typedef struct {
  /* input view */
  const void* x; int64_t x_img_stride; int32_t ldx;
  int32_t N, H_in, W_in, C_in;
  /* filter */
  const void* w; int32_t C_out, R, S;
  /* geometry */
  int32_t stride, transposed, pad_t, pad_l, H_out, W_out;
  /* output view */
  void* y; int64_t y_img_stride; int32_t ldy;
  /* epilogue */
  int32_t epilogue, relu, accumulate;     /* accumulate: y += result (bf16 STORE only)        */
  const float* scale; const float* shift; /* per output channel, may be NULL                 */
  const void* skip; int64_t skip_img_stride; int32_t ld_skip; float rscale;
  float* stats_partial; /* [mbx_conv_stats_rows()][C_out][2] partial sum / sum-of-squares of the stored
                           y (bf16-rounded) for batch-norm statistics, or NULL              */
  int32_t tile_config;  /* 0: the library picks the tile; n > 0: use tile configuration n-1 (0..MBX_CONV_TILE_CONFIGS-1)
                           -- for callers that time the candidates on their own shapes.  Results do not depend on
                           it (same K order), only mbx_conv_stats_rows() does.  For mbx_conv_wgrad*: 0 default,
                           1..6 = {8 waves x 256 blocks, 4 waves x 512, 8 x 192, 4 x 384, 8 x 128, 8 x 224}, 7 / 8 =
                           the narrow tile (64 output channels per block): 8 waves x 256 / 192, 9 / 10 = 4 waves x 512 / 768;
                           11 = un-split (one block per output tile: every dw element is added to once, so the
                           result is bit-reproducible from run to run -- the MBX_DETERMINISTIC debug mode). */
  /* accumulate != 0: y = result + OLD, where OLD is read from acc_src (same shape as y) if it is not NULL, else
     from y itself.  Lets the residual trunk gradient of model.py:21 be built out of place, G[i-1] = G[i] + dgrad,
     so that G[i] survives for the deferred weight gradient of block i's 1x1 "up" convolution.          */
  const void* acc_src; int64_t acc_img_stride; int32_t ld_acc;
  /* Persistent launches (tile_config > 32: conv_igemm5_kernel, one workgroup per CU that walks several tiles): DEVICE
     int32 that is ZERO at launch, or NULL.  With it, a workgroup takes its first tile by position and every further
     tile from this counter (one atomic per tile, fetched two tiles ahead), so a workgroup that starts late -- its CU
     held by another stream's kernels, e.g. RCCL in a data-parallel run -- simply takes fewer tiles; with NULL the tiles
     are dealt statically (first, first + grid, ...) and a late workgroup finishes its share late.  The launch leaves
     the counter advanced: clear it before the next launch that uses it (one fill per step covers a whole table of
     them).  Results are identical either way.                                                                     */
  int32_t* work_counter;
  /* Persistent launches only (tile_config > 32): 0 = one workgroup per CU; n > 0 = at most n workgroups, which leaves
     CUs to a kernel running beside this one on another stream (the capped grouped weight gradient of the previous
     backward segment, mbx_conv_wgrad_grouped_capped; RCCL).  Results do not depend on it.                          */
  int32_t max_workgroups;
  /* tile_config 128 + S (S = 2..32): SPLIT-K for long-K convolutions with few output tiles (forward, bf16 store with or
     without statistics): S slices of the K range per 128 x 64 tile as float32 partial tiles in this workspace
     (mbx_conv_splitk_workspace_bytes(), 16-byte aligned), then one launch that adds the slices in slice order
     (deterministic), rounds, stores y and writes the statistics partials (a row per 16 pixels).  The float32 sum is
     grouped differently from the one-pass kernels: results agree with them to 1 bf16 ulp, not bit for bit.          */
  void* splitk_ws; int64_t splitk_ws_bytes;
  /* stats_rows_mod = R > 0 (round 4): the statistics of a tile are ADDED into row (tile index mod R) of a table
     [R][stats_ld][2] of INT64 that stats_partial then points at (16 bytes per channel and row) and that must be ZERO at
     launch -- R rows whatever the tile shape (mbx_conv_stats_rows() = R), few enough for the consumer to reduce them itself
     (mbx_bn_apply_fused_mapped: no finalize launch), many enough that the adders of one address stay few.  The sums are
     added as 64-bit integers in fixed point (units of 2^-20, resolution 1e-6): integer addition is associative, so the table
     does not depend on the order in which the tiles arrive -- bit-reproducible statistics.  RANGE (round 6): the table is
     exact while a channel's GRAND TOTAL stays in range: |sum y| and sum y^2 over all N H W pixels below 2^42 = 4.4e12 (2^62
     in fixed point; e.g. rms |y| < 1.5e4 on a 64 x 17 x 17 map, < 1.8e3 on 64 x 147 x 147).  Every adder (a pixel tile, a
     workgroup, an image -- the launch knows how many add into one channel) is held to its share 2^42 / adders, so that
     neither a row nor the consumer's sum over the rows can wrap; an adder whose sums are not finite or not below its share
     POISONS the channel -- the sum-of-squares word is forced to INT64_MIN by a signed atomic min, and since the legitimate
     adds are non-negative and total less than 2^62 it stays negative whatever arrives before or after -- and
     mbx_bn_apply_fused_mapped reports NaN mean / rstd for a channel with a negative word or total: out-of-range activations
     end in NaN (as the float32 rows' inf - inf would), never in finite garbage.
     stats_ld (0: C_out): channels per row -- sibling convolutions of a batch-norm group add into channel slices of one
     table (stats_partial then points at the member's first channel).                                              */
  int32_t stats_rows_mod, stats_ld;
  const mbx_bn_bwd_stats* bn_bwd_stats;   /* HOST, may be NULL: see above */
  /* ReLU SIGN BITS of a residual block output (round 4), or NULL: one bit per element, byte [m * ld_bits + c / 8] bit
     (c & 7) = (y[m][c] > 0), m = img * H_out * W_out + pixel, c = channel within this launch's C_out; ld_bits bytes per
     pixel, a multiple of 4 and >= 4 ceil(C_out / 32); the table 4-byte aligned.  MBX_EPI_RESIDUAL with relu: the launch
     WRITES them beside y, four bytes (32 channels) at a time: bytes [0, 4 ceil(C_out / 32)) of every pixel row, zeros for
     channels past C_out.  MBX_EPI_STORE: the launch READS them as the relu-backward mask -- y = (acc [* rscale] [+ OLD]) where the
     bit is set, else 0 -- in place of the `skip` tensor (which must then be NULL): 1/16 of its bytes on a launch that is
     bound by the three tensors its epilogue streams (model.py:19-23 on the way back; train.py:263).  Same results as
     the `skip` form (a NaN in the block output counts as positive here, as not positive there).  Not with the
     stride-2 data gradient, statistics, split-K, the direct launches (96 / 97) or mbx_conv_pair: MBX_ERR_UNSUPPORTED. */
  void* relu_bits; int32_t ld_bits;
  const mbx_bn_apply_desc* bn_apply;      /* HOST, may be NULL: see above (round 6) */
  const mbx_bn_bwd_fused* bn_bwd;         /* HOST, may be NULL: see above (round 6) */
} mbx_conv_desc;
#define MBX_CONV_TILE_CONFIGS 14
/* tile_config beyond the igemm3 tiles 1..MBX_CONV_TILE_CONFIGS: the launch families, described below */
#define MBX_TILE_I5_BASE 32        /* + t + 1 (33..39): the persistent igemm5 launch, tile t */
#define MBX_TILE_I7 65             /* the persistent pointwise launch, filter panel resident in LDS */
#define MBX_TILE_DIRECT3 96        /* the direct 3x3 launch (and the network's first layer) */
#define MBX_TILE_DIRECTW 97        /* the whole-width direct 3x3 launch */
#define MBX_TILE_RESIDENT 98       /* the resident-image launch */
#define MBX_TILE_PWRES 99          /* the pixel-resident pointwise launch */
#define MBX_TILE_SPLITK_BASE 128   /* + S: split-K in S slices, 2 <= S <= MBX_TILE_SPLITK_MAX */
#define MBX_TILE_SPLITK_MAX 32
/* tile_config 33..39: the persistent igemm5 launch (128x64, 128x128, 192x128, 256x128, 256x64, 128x192, 128x256 tiles; 128x192
   without the accumulate + mask epilogue); 65: the persistent
   POINTWISE launch with the filter panel resident in LDS (1x1, unit stride, unpadded, 64 < K <= 384, no statistics; its
   work_counter, if given, is an array of one zeroed int32 per 128-channel column tile, at most 32).  A configuration that
   does not apply returns MBX_ERR_UNSUPPORTED.
   tile_config 96: the DIRECT 3x3 launch (stride 1, forward or data gradient, C_in 32 / 64, C_out <= 64; bf16 store with or
   without statistics, or the affine epilogue) for few channels on large maps: a persistent workgroup per CU stages a pixel
   patch with its halo once and multiplies the nine taps out of LDS instead of gathering the input nine times -- and, under
   the same number, the network's first layer (3x3 / stride 2, C_in 8 = the packed RGB input, C_out <= 32; forward only).
   tile_config 97: the same scheme with WHOLE-WIDTH tiles for narrow maps (8..64 wide: block35's 35 x 35 layers; C_in 32 /
   48 / 64, C_out <= 64).  Same K order and MFMA grouping as the implicit-GEMM tiles: bit-identical outputs;
   mbx_conv_stats_rows() = one row per workgroup.
   tile_config 98 (round 5): the RESIDENT-IMAGE launch for stride-1, same-size convolutions with a one-dimensional multi-tap
   filter on small maps with many channels -- 1x7 / 7x1 on maps of 65..289 pixels with C_in 128 / 160 / 192 (block17,
   model.py:33-37) and 1x3 / 3x1 on 8 x 8 maps with C_in 192 / 224 / 256 (block8, model.py:53-57), forward or data gradient,
   bf16 store with or without statistics or the affine epilogue: a tile = one whole image (staged in LDS once) x a quarter of
   the output channels, the filter streamed per tap.  Bit-identical outputs; mbx_conv_stats_rows() = N (a row per image).
   tile_config 99 (round 5): the PIXEL-RESIDENT POINTWISE launch (1x1, unit stride, unpadded, C_in 96 / 128 / 320 / 384 / 448)
   for the residual epilogue (+ relu, + sign bits) or a store masked by relu sign bits (with or without an accumulate
   source): a 160- / 128-pixel tile resident in LDS, the filter streamed per 128 output channels.  Bit-identical outputs; no
   statistics.  (Built, tested and level with the persistent tiles at BATCH_SIZE 64: not chosen by the engine's rules.) */

int mbx_conv_stats_rows(const mbx_conv_desc* desc /*HOST*/); /* rows of stats_partial */
int mbx_conv(const mbx_conv_desc* desc /*HOST*/, mbx_stream_t stream);
/* Every check of mbx_conv for this descriptor -- arguments, ranges, whether desc->tile_config applies to the shape and
 * epilogue -- WITHOUT a launch: what mbx_conv would return short of a launch error.  For callers that keep a table of
 * measured tile choices and must not find out in the middle of a step that an entry no longer applies.               */
int mbx_conv_supported(const mbx_conv_desc* desc /*HOST*/);
/* TWO independent convolutions in ONE launch (sibling branches that do not fill the chip on their own: block35's two 3x3
 * convolutions, forward and data gradient).  Applies when both descriptors resolve to the same 4-wave 128x64 / 64x64 tile
 * with a store or store + statistics epilogue and general (non-pointwise, non stride-2-gradient) addressing; otherwise
 * MBX_ERR_UNSUPPORTED and nothing is launched (the caller then issues two mbx_conv).  Bit-identical to two mbx_conv.     */
int mbx_conv_pair(const mbx_conv_desc* a /*HOST*/, const mbx_conv_desc* b /*HOST*/, mbx_stream_t stream);
size_t mbx_conv_splitk_workspace_bytes(const mbx_conv_desc* desc /*HOST*/);   /* 0 unless tile_config is a split-K one */

/* Weight gradient (TF autodiff of slim.conv2d, train.py:263):
 * dw[k][r][s][c] += sum_{n,oh,ow} dy[n,oh,ow,k] * x[n, oh*stride-pad_t+r, ow*stride-pad_l+s, c]
 * dw is float32 KRSC, ACCUMULATED with atomics (zero it first).  desc gives x / geometry as
 * in the forward call; dy is an [N,H_out,W_out,C_out] bf16 view.  `db` (float32 [C_out],
 * may be NULL) accumulates sum dy for a bias gradient.                                     */
int mbx_conv_wgrad(const mbx_conv_desc* desc /*HOST: x, geometry, C_out*/, const void* dy,
                   int64_t dy_img_stride, int32_t ld_dy, float* dw, float* db, mbx_stream_t stream);

/* GROUPED weight gradient: the weight gradients of many layers (a whole backward segment) in ONE launch.  dW is
 * only consumed by the optimiser, so the caller keeps each layer's dy alive and defers the weight gradients to the
 * end of a segment: the launch walks a table of work items (layer, output tile, pixel range) built once by
 * mbx_wgrad_plan.  With hundreds of tiles in flight a tile's pixel reduction is split across blocks only when it
 * is longer than a fair share of one CU's work, so most dw elements have a single adder; flag
 * MBX_WGRAD_DETERMINISTIC forbids every split (bit-reproducible dw).  Semantics per job = mbx_conv_wgrad_scaled,
 * with one difference: dw / db MUST be zero before the launch and each job needs its own dw -- a tile whose pixel
 * reduction is not split is written with plain stores (one adder: nothing to add to), split tiles add atomically.
 * The launch is PERSISTENT: one 1024-thread workgroup per CU (8 MFMA waves + 8 LDS-DMA loader waves, 128 VGPRs per lane,
 * 144 KB + 16 B of dynamic LDS: three ring stages of up to six 8 KB sub-images; nothing else fits beside it) pulls work items
 * from per-XCD queues inside the image (the queue heads start at zero in the image and the kernel's last block
 * resets them, so the same image serves every launch; one launch of an image at a time).
 * mbx_wgrad_plan writes a HOST image of mbx_wgrad_plan_bytes() bytes; copy it to 16-byte aligned device memory
 * once and pass that pointer to every launch.  The image embeds the jobs' device pointers.                    */
typedef struct {
  mbx_conv_desc desc;      /* x, geometry, C_out as for mbx_conv_wgrad */
  const void* dy; int64_t dy_img_stride; int32_t ld_dy;
  float scale;             /* multiplies this job's dw / db contributions */
  float* dw; float* db;    /* float32, ACCUMULATED (zero first); db may be NULL */
} mbx_wgrad_job;
typedef struct {
  int32_t n_layers, n_items;
  int64_t layers_off, items_off;   /* byte offsets of the two tables inside the image */
  int64_t queues_off, heads_off;   /* per-XCD work queues: item ranges, and the queue heads the launch advances */
  double flops;                    /* 2 * M * C_out * R*S*C_in summed over the jobs */
  int64_t tally_off;               /* two uint64 the launches only ever add to: work items processed, launches completed;
                                      after a synchronise items == launches * n_items, or a launch has skipped work */
} mbx_wgrad_plan_info;
#define MBX_WGRAD_DETERMINISTIC 1
#define MBX_WGRAD_SCATTER 2        /* A/B knob: deal single items round-robin to the queues (no L2 panel sharing) */
size_t mbx_wgrad_plan_bytes(const mbx_wgrad_job* jobs /*HOST*/, int n_jobs, int flags);
int mbx_wgrad_plan(const mbx_wgrad_job* jobs /*HOST*/, int n_jobs, int flags, void* host_image, size_t bytes,
                   mbx_wgrad_plan_info* info /*HOST, out*/);
int mbx_conv_wgrad_grouped(void* device_image /*queue heads are written*/, const mbx_wgrad_plan_info* info /*HOST*/,
                           mbx_stream_t stream);
/* The same launch with at most max_workgroups persistent workgroups (<= 0: one per CU).  The weight gradient is off the
 * critical path of the backward pass (only the optimiser reads dW): launched on a second stream with a capped grid it
 * runs BESIDE the next segment's data-gradient / batch-norm chain on the CUs that chain leaves idle; any number of
 * workgroups drains the queues (placement is for speed only), results are those of the uncapped launch.            */
int mbx_conv_wgrad_grouped_capped(void* device_image, const mbx_wgrad_plan_info* info /*HOST*/, int max_workgroups,
                                  mbx_stream_t stream);

/* Scalars on the dgrad/wgrad path: mbx_conv multiplies the accumulator by `rscale` when
 * epilogue == MBX_EPI_STORE and rscale != 0 (the residual branch scale of model.py:21 on the
 * way back); mbx_conv_wgrad_scaled multiplies dw/db contributions by `scale`.             */
int mbx_conv_wgrad_scaled(const mbx_conv_desc* desc, const void* dy, int64_t dy_img_stride,
                          int32_t ld_dy, float scale, float* dw, float* db, mbx_stream_t stream);

/* ----------------------------------------------------------------- batch norm (K8, A3)
 * slim.batch_norm as the reference configures it (train.py:94-99): no gamma
 * (scale=False), beta, epsilon 0.001, batch statistics over N*H*W when training, moving
 * averages updated as moving -= (1-decay)*(moving - batch) (biased variance).
 * Forward training = mbx_conv(stats_partial) -> mbx_bn_finalize -> mbx_bn_apply.          */
/* decay < 0 ("store mode", also mbx_bn_apply_fused): moving_mean / moving_var are OVERWRITTEN with the batch mean and the
 * biased batch variance instead of being updated -- for callers that apply the moving-average update later, gated by
 * the step control word (mbx_bn_moving_update below), so that a step the optimiser skips leaves them untouched.      */
int mbx_bn_finalize(const float* stats_partial /*[rows,C,2]*/, int rows, int C, int64_t count,
                    float eps, float decay, float* mean /*[C]*/, float* rstd /*[C]*/,
                    float* moving_mean /*[C] or NULL*/, float* moving_var /*[C] or NULL*/,
                    mbx_stream_t stream);
/* a = relu?((y - mean) * rstd + beta): y bf16 [M,C] contiguous -> a bf16 view (ld_a).     */
int mbx_bn_apply(const void* y, int64_t M, int C, const float* mean, const float* rstd,
                 const float* beta, int relu, void* a, int ld_a, mbx_stream_t stream);
/* mbx_bn_finalize + mbx_bn_apply in ONE launch (each workgroup re-reduces the partials of its own 64
 * channels; used when rows <= 16, otherwise it issues the two launches: re-reducing hundreds of partial
 * rows per workgroup measured slower than the extra launch).  Same results either way.                          */
int mbx_bn_apply_fused(const float* stats_partial, int rows, int64_t count, float eps, float decay,
                       const void* y, int64_t M, int C, const float* beta, int relu, void* a, int ld_a,
                       float* mean, float* rstd, float* moving_mean, float* moving_var,
                       mbx_stream_t stream);
/* Finalize + apply in one launch for a convolution that ADDED its statistics into few rows (mbx_conv_desc.stats_rows_mod:
 * stats_fixed = that INT64 fixed-point table [rows][C][2], rows <= 16, C <= 2048; every workgroup reduces the rows of all
 * C channels itself, then sweeps whole rows of y), with the activation view addressed through a group's channel map (NULL:
 * the identity; see BATCH-NORM GROUPS below).
 * relu_thr ([C], may be NULL): the ReLU threshold on y, mean - beta / rstd (-inf without relu): (y - mean) rstd + beta > 0
 * <=> y > relu_thr -- what mbx_conv's BN-backward statistics epilogue masks with.                                      */
int mbx_bn_apply_fused_mapped(const void* stats_fixed, int rows, int64_t count, float eps, float decay,
                              const void* y, int64_t M, int C, const float* beta, int relu, void* a, int ld_a,
                              const struct mbx_chan_map_s* a_map /*HOST*/, float* mean, float* rstd, float* moving_mean,
                              float* moving_var, float* relu_thr, mbx_stream_t stream);
/* moving -= (1-decay)*(moving - batch) for n channels (every batch-norm layer of a step in one launch; batch_mean /
 * batch_var as written by the store mode above: the same float32 expressions, bit-identical to the in-place update).
 * skip_ctl (DEVICE, two float32, may be NULL): the step control block of mbx_rmsprop_ema_step -- if either word is
 * non-zero the launch changes nothing except *skipped_steps += 1 (DEVICE uint64, may be NULL): a poisoned step or a
 * step after a stop request is skipped EVERYWHERE, moving statistics included (train.py:94-99 updates them as part of
 * the train op, which the reference's py_func error aborts as a whole, loss.py:82).
 * ema_mean / ema_var (may be NULL): the ExponentialMovingAverage shadows of the two (train.py:253-259), updated from the
 * NEW values in the same launch: ema -= (1-ema_decay)*(ema - moving) -- mbx_ema_update's expression.                  */
int mbx_bn_moving_update(float* moving_mean, float* moving_var, const float* batch_mean, const float* batch_var,
                         int64_t n, float decay, const float* skip_ctl, uint64_t* skipped_steps,
                         float* ema_mean, float* ema_var, float ema_decay, mbx_stream_t stream);
/* BATCH-NORM GROUPS.  Sibling convolutions (same pixels, independent inputs: the two 3x3 branches of a block35,
 * model.py:11-17; the stride-2 branches of Mixed_7a, model.py:166-178) are normalised by ONE set of launches: their
 * pre-BN outputs are channel slices of one contiguous [M, C] tensor (each convolution writes its slice: ldy = C), beta /
 * mean / rstd / moving statistics are contiguous in member order, and the activation / gradient VIEW places the members'
 * channels wherever the concat layout wants them: channel c of the [M, C] tensor is channel c + offset[i] of the view,
 * i = the last entry with c_begin[i] <= c.  c_begin ascending from 0, everything a multiple of 8, offsets >= 0 (the
 * view pointer is that of the lowest member).  map = NULL: the identity.  A kernel costs >= 4.4 us in the replayed
 * step whatever it does; a group of two saves a finalize, an apply and a backward launch per step and block.          */
typedef struct mbx_chan_map_s { int32_t n; int32_t c_begin[4]; int32_t offset[4]; } mbx_chan_map;
/* mbx_bn_finalize over up to 4 members: member p's convolution wrote parts[p] = [rows[p]][Cs[p]][2]. */
int mbx_bn_finalize_parts(const float* const* parts /*HOST array of DEVICE pointers*/, const int32_t* rows /*HOST*/,
                          const int32_t* Cs /*HOST*/, int n_parts, int64_t count, float eps, float decay, float* mean,
                          float* rstd, float* moving_mean, float* moving_var, mbx_stream_t stream);
int mbx_bn_apply_mapped(const void* y, int64_t M, int C, const float* mean, const float* rstd, const float* beta,
                        int relu, void* a, int ld_a, const mbx_chan_map* a_map /*HOST*/, mbx_stream_t stream);
/* mbx_bn_apply followed by mbx_maxpool_fwd (3x3, stride 2, VALID) in ONE pass, for a layer whose activation feeds only that
 * pool (the two stem pools, model.py:103,115): p[n,oh,ow,c] = max over the window of bf16(relu?((y - mean) rstd + beta)),
 * argmax = the first maximum's tap (uint8 [N,Ho,Wo,C], may be NULL) -- the activation itself is never stored.
 * y: bf16 [N*H*W, C] contiguous.  Bit-identical to the two calls.                                                       */
int mbx_bn_apply_maxpool(const void* y, int N, int H, int W, int C, const float* mean, const float* rstd, const float* beta,
                         int relu, void* p, int64_t p_img_stride, int ld_p, int Ho, int Wo, uint8_t* argmax,
                         mbx_stream_t stream);
/* Frozen BN folded into the conv epilogue (detect.py:313-326, train.py:124-131):
 * scale = 1/sqrt(moving_var+eps), shift = beta - moving_mean*scale.                       */
int mbx_bn_fold(const float* moving_mean, const float* moving_var, const float* beta, float eps,
                int C, float* scale, float* shift, mbx_stream_t stream);
/* Backward through relu + batch norm.  xhat = (y-mean)*rstd;  g = da * (a > 0) (relu) -- or, when
 * relu != 0 and a == NULL, g = da * (xhat + beta > 0): the mask is recomputed from y with the forward
 * expression, so the activation is not read at all (`beta` is only needed for that form).
 * pass 1 writes partial sums {sum g, sum g*xhat} [rows,C,2]; mbx_bn_bwd_finalize reduces them,
 * ACCUMULATES dbeta += sum g and stores m1 = sum g / M, m2 = sum g*xhat / M;
 * pass 2: dy = rstd * (g - m1 - xhat*m2)  (bf16 [M,C]).                                          */
int mbx_bn_bwd_rows(int64_t M, int C);
int mbx_bn_bwd_reduce(const void* da, int ld_da, const void* a, int ld_a, int relu, const void* y,
                      int64_t M, int C, const float* mean, const float* rstd, const float* beta,
                      float* partial /*[mbx_bn_bwd_rows,C,2]*/, mbx_stream_t stream);
int mbx_bn_bwd_finalize(const float* partial, int rows, int C, int64_t M, float* dbeta /*[C] +=*/,
                        float* m12 /*[2,C]*/, mbx_stream_t stream);
int mbx_bn_bwd_apply(const void* da, int ld_da, const void* a, int ld_a, int relu, const void* y,
                     int64_t M, int C, const float* mean, const float* rstd, const float* beta,
                     const float* m12, void* dy /*bf16 [M,C]*/, mbx_stream_t stream);

/* ... with the gradient view `da` addressed through a group's channel map (a must be NULL: mask from y) */
int mbx_bn_bwd_reduce_mapped(const void* da, int ld_da, const void* a, int ld_a, int relu, const void* y, int64_t M, int C,
                             const float* mean, const float* rstd, const float* beta, float* partial,
                             const mbx_chan_map* da_map /*HOST*/, mbx_stream_t stream);
int mbx_bn_bwd_apply_mapped(const void* da, int ld_da, const void* a, int ld_a, int relu, const void* y, int64_t M, int C,
                            const float* mean, const float* rstd, const float* beta, const float* m12, void* dy,
                            const mbx_chan_map* da_map /*HOST*/, mbx_stream_t stream);

/* Backward through relu + batch norm as ONE STREAMING launch, for a layer whose sums {sum g, sum g y} were ADDED into
 * `rows` rows of stats = [rows][C][2] by the data gradient(s) that wrote da (mbx_bn_bwd_stats above): every workgroup
 * reduces the rows of all C channels itself, then dy = rstd (g - m1 - xhat m2) with g = (y > relu_thr) ? da : 0,
 * m1 = sum g / M, m2 = rstd (sum g y - mean sum g) / M; dbeta [C] += sum g (may be NULL).  No grid barrier, no
 * workspace to time out on: the same launch with and without a concurrent stream.  da through a group's channel map
 * (NULL: identity).  C <= 2048, rows <= 16.                                                                       */
int mbx_bn_bwd_apply_rows(const float* stats, int rows, const void* da, int ld_da, const void* y, int64_t M, int C,
                          const float* mean, const float* rstd, const float* relu_thr, float* dbeta, void* dy,
                          const mbx_chan_map* da_map /*HOST*/, mbx_stream_t stream);

/* The same backward pass in ONE launch (relu mask recomputed from y): every workgroup keeps its slice of
 * (da, y) in registers across a grid barrier, so da and y are read once.  Available when the layer fits
 * one resident workgroup per CU (mbx_bn_bwd_onepass_supported; everything but the 5 stem layers at
 * BATCH_SIZE 64); otherwise MBX_ERR_UNSUPPORTED and the caller uses the three launches above.
 * `ws` (mbx_bn_bwd_onepass_workspace_bytes(C), 16-byte aligned) must be ZERO at launch; after the launch word
 * [8*2*C] (behind the eight accumulator copies) holds the grid size and word [8*2*C + 1] a barrier-timeout flag (0 unless the grid was not resident);
 * a workgroup that timed out also writes NaN into its part of dy (and dbeta), so a step cannot continue silently on
 * partial totals.  dbeta [C] += sum g (may be NULL).  max_workgroups: 0 = one
 * workgroup per CU; a smaller positive number leaves CUs free for a concurrent stream (e.g. an RCCL
 * all-reduce in flight), whose kernels would otherwise delay the barrier until they finish.
 * step_poison (float32 scalar, may be NULL): += 1 per workgroup that timed out -- the first word of the step control
 * block that mbx_rmsprop_ema_step / mbx_ema_update test (skip_ctl), so that a poisoned step is never applied.      */
size_t mbx_bn_bwd_onepass_workspace_bytes(int C);
int mbx_bn_bwd_onepass_supported(int64_t M, int C, int max_workgroups);
int mbx_bn_bwd_onepass(const void* da, int ld_da, int relu, const void* y, int64_t M, int C,
                       const float* mean, const float* rstd, const float* beta, float* dbeta /*[C] +=*/,
                       void* dy /*bf16 [M,C]*/, void* ws, int max_workgroups, float* step_poison /*or NULL*/,
                       mbx_stream_t stream);

/* Three-launch backward of a layer whose activation feeds ONLY a 3x3 / stride-2 VALID max-pool (the two stem pools,
 * model.py:103,115: 177 MB and 124 MB tensors): the activation gradient is gathered from the pool's output gradient gy
 * [N,Ho,Wo,C] and its argmax bytes on the fly (mbx_maxpool_bwd's arithmetic, rounded to bf16 as it would store it: the
 * per-element values are those of mbx_maxpool_bwd; the statistics partials are grouped by 2 x 2 pixel blocks, so the
 * sums agree with mbx_bn_bwd_reduce to float32 rounding), so the max-pool backward launch, the write of its result and
 * the two reads of it disappear.  y / dy: [N*H*W, C] contiguous; relu mask from y; partial rows: mbx_bn_bwd_rows_pooled. */
int mbx_bn_bwd_rows_pooled(int N, int H, int W, int C);
int mbx_bn_bwd_reduce_pooled(const void* gy, int64_t gy_img_stride, int ld_gy, const uint8_t* argmax, int N, int H, int W,
                             int Ho, int Wo, int relu, const void* y, int C, const float* mean, const float* rstd,
                             const float* beta, float* partial /*[mbx_bn_bwd_rows_pooled(N,H,W,C), C, 2]*/, mbx_stream_t stream);
int mbx_bn_bwd_apply_pooled(const void* gy, int64_t gy_img_stride, int ld_gy, const uint8_t* argmax, int N, int H, int W,
                            int Ho, int Wo, int relu, const void* y, int C, const float* mean, const float* rstd,
                            const float* beta, const float* m12, void* dy, mbx_stream_t stream);
int mbx_bn_bwd_onepass_mapped(const void* da, int ld_da, int relu, const void* y, int64_t M, int C, const float* mean,
                              const float* rstd, const float* beta, float* dbeta, void* dy, void* ws, int max_workgroups,
                              float* step_poison, const mbx_chan_map* da_map /*HOST*/, mbx_stream_t stream);

/* ---------------------------------------------------------------------- pooling (K9)
 * NHWC bf16 views.  max: k x k, stride, VALID (model.py:103,115,157,180); argmax (uint8 tap
 * index, first maximum) is kept for the backward pass.  avg: k x k stride 1, pad `pad`
 * on every side, divisor = number of valid taps (TF SAME semantics, model.py:134; VALID
 * 8x8 of model.py:285 with pad 0).  Backward passes gather, `accumulate` adds to dx.      */
int mbx_maxpool_fwd(const void* x, int64_t x_img_stride, int ldx, int N, int H, int W, int C,
                    int k, int stride, void* y, int64_t y_img_stride, int ldy, int Ho, int Wo,
                    uint8_t* argmax /*[N,Ho,Wo,C] or NULL*/, mbx_stream_t stream);
int mbx_maxpool_bwd(const void* dy, int64_t dy_img_stride, int ld_dy, const uint8_t* argmax,
                    int N, int H, int W, int C, int k, int stride, int Ho, int Wo, void* dx,
                    int64_t dx_img_stride, int ld_dx, int accumulate, mbx_stream_t stream);
int mbx_avgpool_fwd(const void* x, int64_t x_img_stride, int ldx, int N, int H, int W, int C,
                    int k, int pad, void* y, int64_t y_img_stride, int ldy, int Ho, int Wo,
                    mbx_stream_t stream);
int mbx_avgpool_bwd(const void* dy, int64_t dy_img_stride, int ld_dy, int N, int H, int W, int C,
                    int k, int pad, int Ho, int Wo, void* dx, int64_t dx_img_stride, int ld_dx,
                    int accumulate, mbx_stream_t stream);

/* ------------------------------------------------------------------- small glue kernels
 * relu backward in place: g *= (a > 0)   (model.py:22-23 on the way back).                 */
int mbx_relu_mask(void* g, int ld_g, const void* a, int ld_a, int64_t M, int C, mbx_stream_t stream);
/* images float32 [N,H,W,3] -> bf16 [N,H,W,8] (channels 3..7 zero) for the stem conv.       */
int mbx_pack_input(const float* img, int64_t pixels, void* out, mbx_stream_t stream);
/* Detection heads (model.py:295-322): one head's float32 conv output h [N*cells, ld_h]
 * (channels [0,4k) locations, [4k,5k) confidence logits) <-> locations [N,P,4],
 * logits [N,P] at prior offset `off` (flatten order of model.py:296-319).
 * scatter writes the bf16 gradient [N*cells, ld_g] (zero beyond 5k) from d_locs/d_logits.  */
int mbx_head_gather(const float* h, int ld_h, int N, int cells, int k, int P, int off,
                    float* locs, float* logits, mbx_stream_t stream);
int mbx_head_scatter(const float* d_locs, const float* d_logits, int N, int cells, int k, int P,
                     int off, void* g, int ld_g, mbx_stream_t stream);

/* All heads of the network in ONE launch each way (at most 8; model.py:198-324 has six): the per-head calls above cost a
 * kernel launch each for a few kilobytes.  `h` / `ld_h` are read by the gather, `g` / `ld_g` written by the scatter.  */
typedef struct {
  const float* h; int32_t ld_h;   /* float32 conv output [N*cells, ld_h] */
  void* g; int32_t ld_g;          /* bf16 gradient [N*cells, ld_g] */
  int32_t cells, k, off;          /* grid cells, boxes per cell, prior offset of the head */
} mbx_head;
int mbx_head_gather_all(const mbx_head* heads /*HOST*/, int n_heads, int N, int P, float* locs, float* logits,
                        mbx_stream_t stream);
int mbx_head_scatter_all(const float* d_locs, const float* d_logits, const mbx_head* heads /*HOST*/, int n_heads, int N,
                         int P, mbx_stream_t stream);

/* Start of a training step's backward pass in one launch: grads[0, n_grads) and bn_ws[0, n_ws) (float32 counts, multiples
 * of 4, 16-byte aligned buffers) are cleared; before grads[ctl_index] -- word [0] of the step control block, the grid-
 * barrier time-outs of the PREVIOUS step (mbx_bn_bwd_onepass step_poison, summed over ranks) -- is cleared, its value is
 * added to *timeouts_total (DEVICE uint64, may be NULL), so that a time-out between two host checks is not lost.
 * zero_scalar (float32, may be NULL) is cleared too: the reg_loss accumulator mbx_rmsprop_ema_step adds to.              */
int mbx_step_begin(float* grads, int64_t n_grads, float* bn_ws, int64_t n_ws, int64_t ctl_index, uint64_t* timeouts_total,
                   float* zero_scalar, mbx_stream_t stream);

/* ---------------------------------------------------------- parameters (A8, K16-K18)
 * Filters live as float32 masters in one flat buffer (KRSC each); the bf16 copies the
 * kernels read are refreshed once per step.  mbx_filter_prepare writes, for every table
 * entry, the flipped channel-transposed dgrad copy [C][R][S][Kpad] from the bf16 KRSC copy. */
typedef struct {
  int64_t src_off;  /* element offset of the KRSC filter in the bf16 flat buffer           */
  int64_t dst_off;  /* element offset of the [C][R][S][Kpad] copy in the dgrad buffer       */
  int32_t K, R, S, C, Kpad;
  int32_t first_block; /* prefix sum of R*S*ceil(C/32)*ceil(Kpad/64) over the entries            */
} mbx_filter_entry;
int mbx_filter_prepare(const void* w_bf16, void* w_dgrad, const mbx_filter_entry* table /*DEVICE*/,
                       int n_entries, int total_blocks, mbx_stream_t stream);

/* RMSProp (tf.train.RMSPropOptimizer, train.py:207-212) + L2 regulariser gradient
 * (train.py:104-105: g += wd*w) + EMA of the variables (train.py:253-259) + refresh of the
 * bf16 copy, one pass over a flat parameter range:
 *   ema -= (1-ema_decay)*(ema - w)   [value before this step's update]
 *   g' = g + wd*w ; ms = decay*ms + (1-decay)*g'^2 ; mom = momentum*mom + lr*g'/sqrt(ms+eps)
 *   w -= mom ; w_bf16 = bf16(w)
 * reg_loss (float32 scalar, may be NULL) += wd/2 * sum w^2 (the value before the update:
 * slim's regularization loss in total_loss, train.py:246).  `trainable` = 0 skips the
 * update (frozen variables still get EMA, regulariser and bf16 refresh).
 * skip_ctl (DEVICE, two float32, may be NULL): the step control block -- [0] barrier timeouts of this step's
 * one-launch BN backward (mbx_bn_bwd_onepass step_poison), [1] ranks that asked to stop; data-parallel callers sum
 * it over ranks together with the gradients.  If either word is non-zero the launch does NOTHING (no update, no
 * EMA, no regulariser, no bf16 refresh): the step is skipped identically on every rank.      */
int mbx_rmsprop_ema_step(float* w, const float* g, float* ms, float* mom /*NULL if momentum==0*/,
                         float* ema /*or NULL*/, void* w_bf16 /*or NULL*/, int64_t n, float lr,
                         float decay, float momentum, float eps, float wd, float ema_decay,
                         int trainable, float* reg_loss, const float* skip_ctl, mbx_stream_t stream);
int mbx_ema_update(float* ema, const float* value, int64_t n, float ema_decay, const float* skip_ctl /*as above*/,
                   mbx_stream_t stream);

/* Global-norm gradient clipping and the non-finite-step guard (not in the reference; nothing here runs unless asked for).
 * The clipped quantity is the vector the optimiser consumes, g' = g + wd*w of mbx_rmsprop_ema_step (g' = g where wd = 0):
 * what tf.clip_by_global_norm would see on the reference's total_loss, which contains slim's regulariser.  Three steps,
 * no host synchronisation, no floating-point atomics -- the same inputs give the same bits:
 *
 * mbx_grad_sqnorm: partials[b] = sum over the elements workgroup b owns of (double)g'^2, for one flat range of n elements;
 *   g' is formed in float32 by the optimiser's own device expression, widened, squared and summed in double (per lane, then
 *   wavefront, then workgroup).  It writes mbx_grad_sqnorm_partials(n) slots (a fixed function of n: ceil(ceil(n/4)/256)
 *   capped at 2048; lane t of workgroup b owns the 16-byte groups b*256 + t + j * 256 * slots, j = 0, 1, ..., and the same
 *   stride over the n % 4 tail -- element by element throughout when g or w is not 16-byte aligned).  w must be given when
 *   wd != 0 and is ignored (may be NULL) when wd == 0.  partials: DEVICE, 8-byte aligned.
 *
 * mbx_clip_finalize: one workgroup sums partials[0, n_slots) -- the slots of every range, in a fixed order -- and writes the
 *   CLIP BLOCK clip[0..8) (DEVICE float32) from total, norm = sqrt(total) and max_norm (> 0; INFINITY = never clip, only
 *   guard), everything computed in double:
 *     clip[0] = ctl[0]                      clip[1] = ctl[1] + (total is Inf or NaN ? 1 : 0)
 *     clip[2] = scale = norm > max_norm ? max_norm / norm : exactly 1.0f   (1.0f for a norm of 0 and for a non-finite total)
 *     clip[3] = (float)norm, before clipping          clip[4] = norm > max_norm ? 1 : 0          clip[5..8) = 0
 *   ctl is the step control block (two float32, see mbx_rmsprop_ema_step); it is only read.  Words [0], [1] make the clip
 *   block a drop-in skip_ctl: every gated launch that is handed the clip block instead of ctl (mbx_rmsprop_ema_step_clipped,
 *   mbx_bn_moving_update, mbx_ema_update) skips a step with a non-finite gradient exactly as it skips a flagged one.
 *   counts (DEVICE int64[2]): counts[0] += 1 when the step is clipped, counts[1] += 1 when its total is non-finite; neither
 *   when ctl was already flagged (that step's gradients are poisoned by design and the skip has its cause).
 *
 * mbx_rmsprop_ema_step_clipped: mbx_rmsprop_ema_step with the clip block in the place of skip_ctl (required); the trainable
 *   branch uses clip[2] * g'.  With clip[2] == 1.0f every result is byte-identical to mbx_rmsprop_ema_step's.              */
int64_t mbx_grad_sqnorm_partials(int64_t n);
int mbx_grad_sqnorm(const float* g, const float* w /*NULL if wd == 0*/, int64_t n, float wd, double* partials,
                    mbx_stream_t stream);
int mbx_clip_finalize(const double* partials, int64_t n_slots, double max_norm, const float* ctl, float* clip /*[8]*/,
                      int64_t* counts /*[2]*/, mbx_stream_t stream);
int mbx_rmsprop_ema_step_clipped(float* w, const float* g, float* ms, float* mom /*NULL if momentum==0*/,
                                 float* ema /*or NULL*/, void* w_bf16 /*or NULL*/, int64_t n, float lr,
                                 float decay, float momentum, float eps, float wd, float ema_decay,
                                 int trainable, float* reg_loss, const float* clip, mbx_stream_t stream);

/* Optimiser choice: momentum SGD, Adam and AdamW beside RMSProp (not in the reference; nothing here runs unless asked for).
 * Both entry points are mbx_rmsprop_ema_step with another element rule: one streaming body gives every rule the same gate,
 * EMA (from the weight before the step), regulariser (reg_loss += wd_l2/2 * sum w^2 when wd_l2 != 0), frozen ranges
 * (trainable = 0: EMA, regulariser and bf16 refresh only), bf16 refresh and 16-byte accesses where every stream is 16-byte
 * aligned.  g' = g + wd_l2*w, the optimiser's one device expression.  ctl (DEVICE, may be NULL when clipped == 0): the step
 * control block; either of its first two words non-zero: the launch does nothing.  clipped != 0: ctl is the CLIP BLOCK of
 * mbx_clip_finalize (required) and g' = clip[2] * g'; a scale of exactly 1.0f changes no bit.
 *
 * mbx_sgd_ema_step (tf.train.MomentumOptimizer): acc = momentum*acc + g' ; w -= lr*acc, or with nesterov != 0
 *   w -= lr*(g' + momentum*acc).  mom is NULL if and only if momentum == 0: then w -= lr*g' and no slot is read or written.
 *
 * mbx_adam_ema_step: m = beta1*m + (1-beta1)*g' ; v = beta2*v + (1-beta2)*g'^2 ;
 *   w -= lr*((m/bc1) / (sqrt(v/bc2) + eps) + wd_decoupled*w), w the value before the step, bc_i = 1 - beta_i^t.
 *   wd_decoupled != 0 is AdamW (callers then pass wd_l2 = 0).  t counts APPLIED steps: t = calls + 1 - (skipped ? *skipped : 0),
 *   calls the host's count of step launches so far and skipped (DEVICE int64, may be NULL) the counter of steps the gate
 *   skipped, as mbx_bn_moving_update maintains it -- read before this step's own increment, which comes later on the stream.
 *   The kernel computes both corrections itself, in double: a skipped step never shifts them and the host never synchronises.
 *   As computed: c_i = (float)(1 / bc_i), the reciprocal formed in double and rounded to float32 once per thread, then per
 *   element m^ = m*c1, v^ = v*c2 and the step lr*(m^ / (sqrtf(v^) + eps) + wd_decoupled*w) in float32 -- a multiplication by
 *   the rounded reciprocal in the place of each division by bc_i, one float32 rounding more than the formula above.
 *   CONTRACT: calls >= *skipped (every skipped step was a launch the host counted).  The device cannot report a count that
 *   breaks it, so t < 1 is taken for t = 1, which keeps the powers and the reciprocals defined; the update is then that of
 *   a first step and is NOT the caller's intent -- the caller keeps its count consistent (Trainer: set_optimizer_steps, and
 *   an assertion on the launch count).
 *
 * MBX_ERR_INVALID_ARG before any device work: n < 0, a null w, a null g (or m, v) with trainable != 0, mom given with momentum
 * == 0 or missing otherwise, momentum or a beta outside [0, 1), eps <= 0, a negative wd_l2 or wd_decoupled, calls < 0, clipped
 * != 0 without ctl; a NaN fails each of these.  n == 0: MBX_OK, nothing launched.
 * Measured (tools/optimizer_bench.py, profiles/optimizer_bench.txt): bytes/s of each rule beside mbx_rmsprop_ema_step in the same
 * graph replays.  What the rules do to AP or convergence on real data is not measured: no dataset or trained model is at hand.  */
int mbx_sgd_ema_step(float* w, const float* g, float* mom /*NULL iff momentum==0*/, float* ema /*or NULL*/,
                     void* w_bf16 /*or NULL*/, int64_t n, float lr, float momentum, int nesterov, float wd_l2, float ema_decay,
                     int trainable, float* reg_loss, const float* ctl, int clipped, mbx_stream_t stream);
int mbx_adam_ema_step(float* w, const float* g, float* m, float* v, float* ema /*or NULL*/, void* w_bf16 /*or NULL*/,
                      int64_t n, float lr, float beta1, float beta2, float eps, float wd_l2, float wd_decoupled, int64_t calls,
                      const int64_t* skipped /*DEVICE, or NULL*/, float ema_decay, int trainable, float* reg_loss,
                      const float* ctl, int clipped, mbx_stream_t stream);

/* Layer-wise trust ratios: LARS on sgd, LAMB on adam / adamw (You, Gitman, Ginsburg 2017; You et al. 2020; not in the
 * reference; nothing here runs unless asked for).  Every VARIABLE of a trainable range gets its own factor
 * r = coeff * ||w|| / ||x||, w the weights before the step and x what the rule would subtract:
 *   sgd          x = g', the optimiser's own g + wd_l2*w in float32, times clip[2] when clipped -- the vector the optimiser
 *                consumes (the paper's denominator ||g|| + wd*||w|| bounds ||g'|| from above).  The rule consumes r*g':
 *                acc = momentum*acc + r*g'.
 *   adam, adamw  x = u = m^ / (sqrt(v^) + eps) + wd_decoupled*w from the UPDATED moments, AdamRule's own expression.  The step
 *                is w -= lr * (r*u).
 * A variable ADAPTS iff the caller says so (Trainer: more than one dimension); r is exactly 1.0f when it does not, or when
 * either norm is 0.  Otherwise r = (float)((double)coeff * sqrt(sum w^2) / sqrt(sum x^2)): both sums in double over float32
 * values, no epsilon, no special case for a non-finite norm (with clipping the guard skips such a step already).
 * A ratio of exactly 1.0f changes no bit: w, the slots, ema and w_bf16 are then byte-identical to mbx_sgd_ema_step /
 * mbx_adam_ema_step on the same range (reg_loss up to the order of its atomics).
 *
 * THE PLAN (host only, no device).  The variables of one range form a contiguous partition: bounds (HOST int64[n_vars + 1],
 * ascending, bounds[0] = 0, range coordinates -- element 0 is what the w, g, ... pointers of the launches point at) and
 * adapt (HOST int32[n_vars]).  Chunks are cut on the grid of multiples of CH = mbx_trust_chunk_elems() (a power of two, a
 * multiple of 1024) AND at every variable bound: a chunk lies in one variable, is at most CH long and starts at a multiple
 * of CH or at a variable bound; chunks are in ascending order, a variable's chunks are consecutive.  mbx_trust_plan_count
 * returns their number, or 0 for arguments mbx_trust_plan refuses; mbx_trust_plan fills chunks_out[count] and
 * vars_out[n_vars], two images the caller uploads once (DEVICE copies 8-byte aligned).
 *
 * THE PASSES, each one workgroup of 256 per chunk (mbx_trust_ratios: one wavefront per variable), all gated like the step: with
 * ctl (the step control block, or the CLIP BLOCK when clipped != 0) flagged NOTHING is written -- moments, partials and ratio
 * keep their contents.  Within a chunk: scalars up to 4-element alignment, 16-byte accesses over the body, scalars for the
 * tail; element by element throughout when a pointer is not 16-byte aligned (w_bf16: 8-byte).  Variable bounds need no
 * alignment at all.
 *   mbx_trust_norms_sgd     partials[2c] = sum w^2, partials[2c + 1] = sum x^2 over chunk c (lane, wavefront, workgroup in a fixed
 *                           order; no atomics: the same inputs give the same bits).  Reads w and g.
 *   mbx_trust_moments_adam  the same two sums with x = u, and WRITES the updated m and v (mbx_adam_ema_step's moments and bias
 *                           correction: calls / skipped as there).
 *   mbx_trust_ratios        ratio[i] (DEVICE float32[n_vars]) from the slots of variable i's chunks, summed in a fixed order.
 *   mbx_sgd_ema_step_trust, mbx_adam_ema_step_trust
 *                           the twins' arguments plus the plan and the ratios: the gate, the EMA from the weight before the
 *                           step, reg_loss, frozen ranges and the bf16 refresh as in the twins.  n is the range's length (0:
 *                           MBX_OK, nothing launched); the elements touched are the chunks'.  The adam form recomputes u from
 *                           the STORED moments and does not update them again: it follows mbx_trust_moments_adam of the same
 *                           step with the same calls / skipped, and does not read g.
 * MBX_ERR_INVALID_ARG before any device work: what the twins refuse; n_vars < 1, a null bounds / adapt / output, bounds not
 * ascending from 0 or with an empty variable; a null or misaligned table, n_chunks or n_vars <= 0 in the norm and ratio passes
 * (n_chunks < 0 in the apply passes), a null partials or ratio, coeff <= 0, infinite or NaN, clipped != 0 without ctl.
 * Measured (tools/trust_bench.py, profiles/trust_bench.txt): each pass beside its partner of the same build.  What LARS / LAMB
 * do to AP or convergence on real data is not measured: no dataset or trained model is at hand.                          */
typedef struct { int64_t lo; int32_t len; int32_t var; } mbx_trust_chunk;                          /* 16 bytes */
typedef struct { int32_t first_chunk; int32_t n_chunks; int32_t adapt; int32_t pad; } mbx_trust_var; /* 16 bytes */
int64_t mbx_trust_chunk_elems(void);
int64_t mbx_trust_plan_count(const int64_t* bounds /*HOST [n_vars+1]*/, int64_t n_vars);
int mbx_trust_plan(const int64_t* bounds /*HOST [n_vars+1]*/, const int32_t* adapt /*HOST [n_vars]*/, int64_t n_vars,
                   mbx_trust_chunk* chunks_out /*HOST*/, mbx_trust_var* vars_out /*HOST*/);
int mbx_trust_norms_sgd(const float* w, const float* g, const mbx_trust_chunk* chunks, int64_t n_chunks, float wd_l2,
                        double* partials /*[2*n_chunks]*/, const float* ctl, int clipped, mbx_stream_t stream);
int mbx_trust_moments_adam(const float* w, const float* g, float* m, float* v, const mbx_trust_chunk* chunks, int64_t n_chunks,
                           float beta1, float beta2, float eps, float wd_l2, float wd_decoupled, int64_t calls,
                           const int64_t* skipped /*DEVICE, or NULL*/, double* partials /*[2*n_chunks]*/, const float* ctl,
                           int clipped, mbx_stream_t stream);
int mbx_trust_ratios(const double* partials, const mbx_trust_var* vars, int64_t n_vars, float coeff, float* ratio /*[n_vars]*/,
                     const float* ctl, mbx_stream_t stream);
int mbx_sgd_ema_step_trust(float* w, const float* g, float* mom /*NULL iff momentum==0*/, float* ema /*or NULL*/,
                           void* w_bf16 /*or NULL*/, int64_t n, float lr, float momentum, int nesterov, float wd_l2,
                           float ema_decay, int trainable, float* reg_loss, const float* ctl, int clipped,
                           const mbx_trust_chunk* chunks, int64_t n_chunks, const float* ratio, mbx_stream_t stream);
int mbx_adam_ema_step_trust(float* w, const float* g, float* m, float* v, float* ema /*or NULL*/, void* w_bf16 /*or NULL*/,
                            int64_t n, float lr, float beta1, float beta2, float eps, float wd_l2, float wd_decoupled,
                            int64_t calls, const int64_t* skipped /*DEVICE, or NULL*/, float ema_decay, int trainable,
                            float* reg_loss, const float* ctl, int clipped, const mbx_trust_chunk* chunks, int64_t n_chunks,
                            const float* ratio, mbx_stream_t stream);

/* ------------------------------------------------------------ training input augmentation (row F1)
 * The pixel half of the reference's training input graph (inputs.py:264-351: crop, tf.image.resize_images with a
 * random ResizeMethod, distort_color, random_flip_left_right, (image - 0.5) * 2) for one batch.  The host draws every
 * random decision and decodes the JPEGs (multibox_amd/inputs.py: plan_augmentation); each item describes one image:
 * its already-cropped pixels [src_h][src_w][3] uint8 at src + src_offset, the resize method (0 bilinear, 1 nearest,
 * 2 bicubic, 3 area: TF 0.11's legacy kernels, align_corners = False; 4 = the bytes at src_offset are a float32
 * [S][S][3] picture in [0,1] the host prepared itself, src_offset a multiple of 4), the colour ops in application
 * order (0 brightness delta, 1 saturation factor, 2 hue delta, 3 contrast factor; n_ops = 0: no colour distortion and
 * no clipping), and the flip.  out[b] = the [S][S][3] float32 picture in [-1,1].
 * any_contrast must be non-zero iff some item has a contrast op (it adds the per-image mean pass).
 * Resize arithmetic is float32 in the host restatement's rounding order (bit-identical to it); colour ops run in
 * float64 like the restatement and differ from it only through the summation order of the contrast mean.          */
typedef struct {
  uint64_t src_offset;
  int32_t src_h, src_w;
  int32_t method;
  int32_t flip;
  int32_t n_ops;
  int32_t op[4];
  int32_t pad_;
  double arg[4];
} mbx_augment_item;                                   /* 80 bytes */
size_t mbx_augment_workspace_bytes(int B, int S);
int mbx_augment_batch(const uint8_t* src /*device*/, const mbx_augment_item* items /*device, [B]*/, int B, int S,
                      int any_contrast, float* out /*[B,S,S,3]*/, void* workspace, mbx_stream_t stream);

/* Detection input (row F3; detect.py:181-281): patch i is a win_h x win_w window at (win_y, win_x) of the decoded
 * image [img_h][img_w][3] uint8 at src + src_offset -- of its left-right mirror image when flip_source -- scaled to
 * [-1,1] first ((x/255 - 0.5) * 2, detect.py:181-182) and then resized to S x S with TF 0.11's legacy bilinear kernel
 * (tf.image.resize_images, align_corners = False).  The whole image as one window gives the original / flipped
 * original patches, the sliding windows of detect.extract_patches (detect.py:20-72) the crops.  The window must lie
 * inside the image (the host checks).  out[i] = float32 [S][S][3]; bit-identical to the host arithmetic.          */
typedef struct {
  uint64_t src_offset;
  int32_t img_h, img_w;
  int32_t win_y, win_x, win_h, win_w;
  int32_t flip_source;
  int32_t pad_;
} mbx_patch_item;                                     /* 40 bytes */
int mbx_extract_patches(const uint8_t* src /*device*/, const mbx_patch_item* items /*device, [n]*/, int n, int S,
                        float* out /*[n,S,S,3]*/, mbx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MBX_H */
