/* include/icet_hip.h -- C ABI of the MI355X-native ICET hot path (libicet_hip.so).
 *
 * This is the drop-in boundary for the ONE path this project accelerates: the body of the reference's
 * `ICET::ICET(...)` constructor (/root/reference/src/icet.cpp:29-63, declared include/icet.h:38-40),
 * i.e. fitScan1 -> prepScan2 -> runlen x fitScan2, whose only outputs the callers read are the public
 * members `X` and `pred_stds` (src/odometry.cpp:76-79,126-131; src/simpleMapMaker.cpp:119-122).
 * The reference has no FFI; a maintainer would bind these entry points from the constructor (see
 * INTEGRATION.md for the exact stub).  Plain pointers and sizes only -- no Eigen, torch or HIP types.
 *
 * Scan layout everywhere: N x 3 float32 COLUMN-MAJOR with leading dimension ld >= N, i.e. exactly
 * `Eigen::MatrixXf::data()` of the reference's `MatrixXf& scan` arguments: x[0..N) | y[0..N) | z[0..N).
 *
 * All entry points return an icet_status; none throws, none aborts.  The library fails loudly
 * (ICET_ERR_NO_DEVICE / ICET_ERR_HIP) when no gfx950 device or kernel image is usable -- there is no
 * CPU fallback behind this ABI.
 */
#ifndef ICET_HIP_H
#define ICET_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum icet_status {
    ICET_OK = 0,
    ICET_ERR_BAD_ARG = 1,     /* null pointer, negative size, ld < n, bins <= 0, ...            */
    ICET_ERR_NO_DEVICE = 2,   /* no HIP device / device id out of range                          */
    ICET_ERR_HIP = 3,         /* a HIP runtime call or kernel launch failed (see icet_last_error) */
    ICET_ERR_NOMEM = 4,       /* device or host allocation failed                                 */
    ICET_ERR_UNSUPPORTED = 5  /* e.g. bins_phi*bins_theta above the voxel limit (10000: the voxel tables of one pair live in one block's LDS) */
} icet_status;

/* Mirrors the reference constructor's scalar arguments (include/icet.h:38-40, defaults n=25,
 * thresh=0.1, buff=0.1; call sites src/odometry.cpp:73-76, src/simpleMapMaker.cpp:113-119). */
typedef struct icet_params {
    int32_t runlen;       /* Gauss-Newton iterations (`runlen`, 7 or 12 at the call sites)       */
    int32_t bins_phi;     /* `num_bins_phi`   : polar-angle ("elevation") bins, 24               */
    int32_t bins_theta;   /* `num_bins_theta` : azimuth bins, 75                                  */
    int32_t n;            /* minimum points per cluster                                           */
    float   thresh;       /* radial jump threshold of findCluster (src/icet.cpp:557)              */
    float   buff;         /* radial buffer added to the cluster bounds                            */
    int32_t flags;        /* ICET_FLAG_* below; 0 = reference behaviour                           */
} icet_params;

enum { ICET_FLAG_NONE = 0,
       ICET_FLAG_TIMING = 1,  /* record HIP events around every bin/accumulate launch (icet_last_timing[2]) */
       ICET_FLAG_TRUE_SORT = 2, /* NON-PARITY EXTENSION: really sort scan 1 by range before clustering, instead of reproducing
                                  the reference's one-step swap loop (src/icet.cpp:78-83), which leaves the rows scrambled so
                                  that findCluster sees most bins in a shuffled order and only ~1/4 of the populated bins get a
                                  Gaussian.  Results then differ from the reference by design (more voxels, better conditioned);
                                  the oracle has the same switch so that the extension is still checked against a CPU twin. */
       ICET_FLAG_REJECT_MOVING = 4, /* NON-PARITY EXTENSION: moving-object rejection as in the reference's Python
                                  variant (python/ICET_spherical.py:175-250, the hard cutoff that is live there): from the 5th iteration on
                                  (start_RM_iter = 4), a voxel whose compact residual L U^T (mu2 - mu1) exceeds RM_thresh = 0.3 m in any
                                  kept axis is left out of that iteration's H^T W H and H^T W dz.  The C++ reference has nothing like it, so
                                  results differ from it by design; the oracle has the same switch (ICET_ORACLE_REJECT_MOVING). */
       ICET_FLAG_HALF_GAP_BOUNDS = 8, /* NON-PARITY EXTENSION: the cluster buffers the reference's Python variant
                                  DESCRIBES ("as described in spherical paper", the comments at python/utils.py:92-119 -- the TensorFlow
                                  code there adds the FULL gap when 2*gap < max_buffer, which is not this rule): the radial bounds of a
                                  voxel's cluster reach half way to the nearest point outside it, at most `buff`, instead of `buff` on either side (a neighbour
                                  that exists is more than `thresh` away, so this only tightens bounds whose neighbour lies within 2 buff).
                                  Needs the voxel's rows in ascending range, so it implies ICET_FLAG_TRUE_SORT.  Oracle twin:
                                  ICET_ORACLE_HALF_GAP. */
       ICET_FLAG_ROUNDTRIP_SCAN2 = 16, /* PARITY-STUDY OPTION (not an extension: it makes the loop MORE literal).  The reference passes scan 2 through
                                  cartesianToSpherical -> sphericalToCartesian twice: once as a whole (points2_OG, src/icet.cpp:275) and, every
                                  iteration, the in-bounds points of every voxel (:303).  Each trip moves a point by 1-2 ulp; the default path
                                  skips both (one of several last-bit triggers behind the pairs that differ from the CPU restatement by
                                  > 5e-5 m; restoring them closes some of those pairs, not all).  With this flag both trips are made, under the shared arithmetic rule (correctly rounded angles and
                                  sines / cosines): a pre-pass over scan 2, and a double-precision atan2 + acos per in-bounds point per
                                  iteration -- about twice the loop time.  Decisions (which voxel, inside the bounds) are unchanged. */
       ICET_FLAG_DOUBLE_W = 32 /* ACCURACY OPTION (the default of rounds 2-5).  The per-voxel weight W = pinv(L U^T R_noise U L^T) (src/icet.cpp:317-321) is, in the reference,
                                  Eigen's float CompleteOrthogonalDecomposition of a float matrix: its result carries a relative error of cond x eps and its rank decision is
                                  the pivot rule.  Since round 6 the device does exactly that by default (Eigen 3.3's algorithm statement by statement on the full, unsymmetrised
                                  3 x 3, bit-identical to the CPU restatement's function on the same matrix: tests test_pinv3_reference_bits).  With this flag W is taken in
                                  DOUBLE with an eigenvalue rank rule instead -- the better-conditioned answer.  On lidar scenes the two agree to rounding; on voxels whose
                                  covariance is thin to the point of cond 1e6 .. 1e7 (millimetre-noise scenes, clusters of three points) they do not: H^T W H differs by 10 %
                                  and more, a condition number at checkCondition's cutoff lands on the other side (other pruned axes, pred_stds of 1e-4 instead of -0.9995),
                                  while the reference's own answer moves by per cents with the last bit of its input. */ };

/* A scan that already lives in device memory (HBM) on the context's device. */
typedef struct icet_dev_scan {
    const float* ptr;     /* device pointer, column-major N x 3, 16-byte aligned                  */
    int64_t n;            /* points                                                               */
    int64_t ld;           /* leading dimension in floats (>= n)                                   */
} icet_dev_scan;

/* Optional side outputs of a single-pair solve: what the reference object exposes besides X and
 * pred_stds (include/icet.h:78-107).  Any pointer may be NULL.  V = bins_phi * bins_theta, voxel
 * row index v = bins_theta * phi + theta (src/icet.cpp:149). */
typedef struct icet_aux {
    float*   cluster_bounds;  /* V x 6 row-major: azMin,azMax,elMin,elMax,inner,outer  (`clusterBounds`) */
    int32_t* n1_raw;          /* V: scan-1 points per angular bin (|pointIndices1[theta][phi]|)          */
    int32_t* has_fit;         /* V: 1 where mu1/sigma1/U/L exist                                          */
    float*   mu1;             /* V x 3   (`mu1`)                                                          */
    float*   sigma1;          /* V x 9   (`sigma1`, row-major 3x3)                                        */
    float*   evecs1;          /* V x 9   eigenvectors as columns (reference stores U = transpose)        */
    float*   l_diag;          /* V x 3   diagonal of `L`                                                  */
    float*   x_hist;          /* runlen x 6: X after every iteration; X before the last update gives
                                 the transform of the reference's final `points2` member               */
    float*   htwh;            /* runlen x 36 (`HTWH_i` per iteration)                                     */
    float*   htwdz;           /* runlen x 6  (`HTWdz_i` per iteration)                                    */
    int32_t* n2_raw;          /* runlen x V: |pointIndices2| (only voxels with a scan-1 fit are counted) */
    int32_t* n2_in;           /* runlen x V: scan-2 points inside the voxel's cluster bounds             */
    float*   test_points;     /* (V x 6) x 3 row-major (`testPoints`, src/icet.cpp:41,213-231): rows 6v + 2k, 6v + 2k + 1 hold
                                 the two sigma points of axis k of voxel v when that axis was pruned (L row k = 0); every
                                 other row is zero (the reference leaves those rows uninitialised)                          */
    float*   points2;         /* n2 x 3 COLUMN-major, leading dimension n2 (`points2`, include/icet.h:80): scan 2 as the last
                                 fitScan2 transformed it, (p + t) * R with the X before the final update (src/icet.cpp:375-378
                                 precede :433), in the CALLER's row order (the device never sorts scan 2); scan 2 itself when runlen == 0 */
    /* The per-point members of the reference object (include/icet.h:79,82,95-96).  No caller in the reference reads them; they cost
     * extra kernels and several MB of D2H, so they are produced only when asked for. */
    float*   points1_spherical; /* n1 x 3 COLUMN-major (r | theta | phi), leading dimension n1 (`points1Spherical`): row p is the scan-1
                                   point that sits at position p after the reference's radial sort + swap loop (src/icet.cpp:69-83)   */
    int32_t* point_index1;      /* n1: `pointIndices1` flattened -- the positions (rows of points1_spherical) of voxel v, ascending,
                                   are point_index1[bin_start1[v] .. bin_start1[v + 1])  (src/icet.cpp:86, 534-554)                   */
    int32_t* bin_start1;        /* V + 1                                                                                              */
    float*   points2_spherical; /* n2 x 3 COLUMN-major (r | theta | phi) of `points2` (`points2Spherical` after the last fitScan2,
                                   src/icet.cpp:387), caller's row order                                                              */
    int32_t* voxel2;            /* n2: the voxel sortSphericalCoordinates assigns to every row of points2 in the last fitScan2
                                   (src/icet.cpp:388): `pointIndices2[theta][phi]` = the rows i with voxel2[i] == T * phi + theta, ascending */
    float*   cond_info;         /* runlen x 8: what ICET::checkCondition (src/icet.cpp:443-492) saw in every iteration: [0,6) the eigenvalues of
                                   HTWH_i ascending (NaN when the Cholesky route proved the matrix well conditioned and never computed them),
                                   [6] the number of pruned axes (rows dropped from L2), [7] the route: 0 Cholesky, 2 the literal restatement */
} icet_aux;

typedef struct icet_ctx icet_ctx;   /* opaque: device id, stream, workspace */

/* Create / destroy a context bound to one device.  `hip_stream` is a hipStream_t passed as void*
 * (NULL = the context creates and owns a non-blocking stream).  One context is not re-entrant; use
 * one per host thread (the reference constructs one ICET object at a time per node: ros::spin()). */
icet_status icet_create(icet_ctx** ctx, int device_id, void* hip_stream);
icet_status icet_destroy(icet_ctx* ctx);
const char* icet_last_error(const icet_ctx* ctx);      /* static/ctx-owned string, never NULL */
const char* icet_version(void);

/* --- the constructor replacement: one scan pair, HOST pointers (copies in, solves, copies out) ----
 * Replaces ICET::ICET (src/icet.cpp:29-63).  x0 = `X0`; x_out = member `X`; pred_stds_out = member
 * `pred_stds`; cov_out (may be NULL) = the 6x6 `noise_mat` local of the last fitScan2
 * (src/icet.cpp:410-411), row-major. */
icet_status icet_solve(icet_ctx* ctx, const icet_params* p,
                       const float* scan1, int64_t n1, int64_t ld1,
                       const float* scan2, int64_t n2, int64_t ld2,
                       const float x0[6], float x_out[6], float pred_stds_out[6], float cov_out[36],
                       icet_aux* aux_or_null);

/* The same call in two halves.  icet_solve_begin enqueues the uploads of both scans, the whole registration and the copy of the
 * results and returns without waiting for the device; icet_solve_end waits and fills x_out / pred_stds_out / cov_out / the aux tables
 * named at begin.  Both scans and every output pointer must stay valid -- the scans unmodified -- until icet_solve_end returns.  Host work placed between the two -- the reference's constructor deep-copies both scans into its members
 * (src/icet.cpp:30,33); include/icet.h makes those copies there -- overlaps with the device.  One begin per context at a time; the
 * other host-pointer entry points refuse to run in between (ICET_ERR_BAD_ARG). */
icet_status icet_solve_begin(icet_ctx* ctx, const icet_params* p,
                             const float* scan1, int64_t n1, int64_t ld1,
                             const float* scan2, int64_t n2, int64_t ld2,
                             const float x0[6], float x_out[6], float pred_stds_out[6], float cov_out[36],
                             icet_aux* aux_or_null);
/* Optional, between begin and end: returns as soon as the KEYFRAME tables named at begin (cluster_bounds, has_fit, mu1, sigma1, evecs1,
 * l_diag, test_points -- everything fitScan1 produces, src/icet.cpp:68-252) are in the caller's arrays, while the Gauss-Newton loop is
 * still iterating on the device: the caller can convert them (include/icet.h builds its Eigen members and std::maps) under the loop. */
icet_status icet_solve_keyframe_tables(icet_ctx* ctx);
icet_status icet_solve_end(icet_ctx* ctx);

/* --- N independent pairs, HOST pointers (one ICET object per pair in the reference) --------------- */
icet_status icet_solve_batch(icet_ctx* ctx, const icet_params* p, int32_t n_pairs,
                             const float* const* scan1, const int64_t* n1,
                             const float* const* scan2, const int64_t* n2,
                             const float* x0 /* n_pairs x 6 or NULL = zeros */,
                             float* x_out /* n_pairs x 6 */, float* pred_stds_out /* n_pairs x 6 */,
                             float* cov_out /* n_pairs x 36 or NULL */);

/* --- N independent pairs, inputs and outputs resident in HBM; asynchronous on the ctx stream ------
 * d_x0: device n_pairs x 6 or NULL (zeros).  d_out: device n_pairs x 48 floats per pair:
 * [0,6) X, [6,12) pred_stds, [12,48) cov row-major.  Returns after enqueueing; call icet_sync. */
icet_status icet_solve_batch_device(icet_ctx* ctx, const icet_params* p, int32_t n_pairs,
                                    const icet_dev_scan* scan1, const icet_dev_scan* scan2,
                                    const float* d_x0, float* d_out);
/* Waits until everything this context has enqueued is done.  Behind exactly one small icet_solve_batch_device call (<= 8 pairs: a replayed graph) it watches a word of
 * pinned memory that the solve's last kernel raises behind its results instead of synchronising the stream (10 us sooner on this part); otherwise hipStreamSynchronize. */
icet_status icet_sync(icet_ctx* ctx);

/* --- the same solve in two halves, for the sequential callers (src/odometry.cpp:73-88: scan 2 of one frame is scan 1 of the next) ---
 * icet_keyframe_device builds the keyframe of n scans -- ICET::fitScan1, src/icet.cpp:68-107 -- and parks it in the context;
 * icet_register_device runs prepScan2 + runlen x fitScan2 (:254-277, :372-436) of n scan-2s against it, with the results of
 * icet_solve_batch_device bit for bit.  Both are asynchronous on the context's stream; a parked keyframe stays valid (and can be
 * registered against again) until the context solves or parks another.  With two contexts a caller builds the keyframe of frame
 * k on one stream while frame k-1 / k still iterates on the other (include/icet_nodes.h does). */
icet_status icet_keyframe_device(icet_ctx* ctx, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan1);
icet_status icet_register_device(icet_ctx* ctx, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan2,
                                 const float* d_x0, float* d_out);

/* The same two halves for scans whose row counts only the DEVICE knows yet (a range filter that compacted them a moment ago on the same
 * stream, src/odometry.cpp:57-70): scan[k].n is an UPPER BOUND (the launch geometry is sized from it), d_rows[k] (device, int32, may be NULL =
 * the bounds are the counts) the actual number of rows, read by the kernels when they run.  The caller need not wait for the filter. */
icet_status icet_keyframe_device_n(icet_ctx* ctx, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan1, const int32_t* d_rows);
icet_status icet_register_device_n(icet_ctx* ctx, const icet_params* p, int32_t n_pairs, const icet_dev_scan* scan2, const int32_t* d_rows,
                                   const float* d_x0, float* d_out);

/* --- many scans against shared parked keyframes: each keyframe is built once, however often it is registered against ---------------
 * Multi-start (one pair from several X0), loop-closure / relocalisation candidates (one scan against K stored keyframes, or K scans against
 * one map keyframe), several sensors against one reference.  Registration r runs prepScan2 + runlen x fitScan2 of scan2[r], from d_x0[r]
 * (NULL = zeros), against parked keyframe kf_index[r] (HOST array, 0 <= kf_index[r] < the parked count; repeats and any order allowed).
 * d_out: n_regs x 48 floats in the layout of icet_solve_batch_device.  Bit for bit the result icet_solve_batch_device gives for the pair
 * (scan1[kf_index[r]], scan2[r], x0[r]).  Asynchronous on the context's stream (icet_sync); kf_index is read before the call returns.
 * The parked keyframe stays parked: it can be registered against again, by this call or icet_register_device.  What un-parks it: a whole
 * solve on the context (icet_solve, icet_solve_begin, icet_solve_batch[_device], icet_solve_indexed), another icet_keyframe_device[_n], and
 * an icet_reserve that has to grow the keyframe side of the workspace (more keyframes, a finer grid or more scan-1 points than any call so far).
 * Growing the registration side -- more registrations or scan-2 points than before -- leaves the keyframe alone.
 * Same argument rules as icet_register_device_n: ICET_ERR_BAD_ARG when no keyframe is parked, when the grid, n, thresh, buff or the
 * keyframe-shaping flags (ICET_FLAG_TRUE_SORT, ICET_FLAG_HALF_GAP_BOUNDS) differ from the parked keyframe's, or when an index is out of range;
 * ICET_ERR_UNSUPPORTED while option "keep" is on (the indexed loop runs the plain point pass).  A refused call leaves the parked keyframe valid.
 * runlen == 0 writes X = X0, pred_stds = cov = 0; n_regs == 0 returns ICET_OK and does nothing.  n_regs may be larger or smaller than the
 * parked count; the limits are those of a batch of n_regs pairs.  ICET_FLAG_ROUNDTRIP_SCAN2, REJECT_MOVING and DOUBLE_W apply per call. */
icet_status icet_register_indexed_device(icet_ctx* ctx, const icet_params* p, int32_t n_regs, const int32_t* kf_index,
                                         const icet_dev_scan* scan2, const float* d_x0, float* d_out);

/* Host-pointer form, shaped like icet_solve_batch: parks the keyframes of the n_kf scan 1s (they stay parked after the call), runs the
 * n_regs registrations and copies the results out (x0: n_regs x 6 or NULL; x_out, pred_stds_out: n_regs x 6; cov_out: n_regs x 36 or NULL). */
icet_status icet_solve_indexed(icet_ctx* ctx, const icet_params* p,
                               int32_t n_kf, const float* const* scan1, const int64_t* n1,
                               int32_t n_regs, const int32_t* kf_index, const float* const* scan2, const int64_t* n2,
                               const float* x0, float* x_out, float* pred_stds_out, float* cov_out);

/* --- how well scan 2 sits on its keyframe at a pose: the registration score ------------------------------------------------------------
 * The quantity the Gauss-Newton step minimises, evaluated at pose X over the voxels and gates of the iteration the loop would run next at X:
 * a slot of the keyframe with a fitted Gaussian whose angular bin holds n2 > n scan-2 points, m > n of them inside the cluster bounds, and --
 * with ICET_FLAG_REJECT_MOVING -- the moving-voxel gate at iteration index p->runlen.  With the loop's own dz = L U^T (mu2 - mu1) and
 * W = pinv(L U^T R_noise U L^T) (float COD, or the double path under ICET_FLAG_DOUBLE_W):
 *     chi2 = sum_v dz^T W dz        voxels = contributing voxels        points_in = sum_v m        points = scan-2 rows
 *     chi2_per_voxel = chi2 / voxels (+inf when voxels == 0)            overlap = points_in / points (0 when points == 0)
 * chi2 is summed in double in a fixed order and rounded once: a registration's score bits do not depend on the other registrations of the call.
 * Lower chi2_per_voxel = better fit; overlap hardly moves between a stuck and a converged solve, so it is no criterion on its own. */
typedef struct icet_score {
    float   chi2, chi2_per_voxel;
    int32_t voxels, points_in, points;
    float   overlap;
    int32_t reserved[2];          /* zero */
} icet_score;                     /* 32 bytes */

/* The score of given poses: registration r = scan2[r] at pose d_X[r] (device, n_regs x 6) against parked keyframe kf_index[r].  Runs no
 * iteration (p->runlen only places the moving-voxel gate); d_score: device, n_regs.  Argument rules, keyframe survival and asynchrony are those
 * of icet_register_indexed_device.  The pose-hypothesis and candidate-verification primitive. */
icet_status icet_score_indexed_device(icet_ctx* ctx, const icet_params* p, int32_t n_regs, const int32_t* kf_index,
                                      const icet_dev_scan* scan2, const float* d_X, icet_score* d_score);
/* icet_register_indexed_device followed by the score at every final X, in one enqueue.  d_out carries exactly the bits of the unscored
 * call; d_score[r] equals icet_score_indexed_device at X = d_out[r][0..6).  runlen == 0 scores X0. */
icet_status icet_register_indexed_scored_device(icet_ctx* ctx, const icet_params* p, int32_t n_regs, const int32_t* kf_index,
                                                const icet_dev_scan* scan2, const float* d_x0, float* d_out, icet_score* d_score);
/* Host-pointer forms, shaped like icet_solve_indexed (the keyframes stay parked).  score_out: n_regs; X: n_regs x 6. */
icet_status icet_solve_indexed_scored(icet_ctx* ctx, const icet_params* p,
                                      int32_t n_kf, const float* const* scan1, const int64_t* n1,
                                      int32_t n_regs, const int32_t* kf_index, const float* const* scan2, const int64_t* n2,
                                      const float* x0, float* x_out, float* pred_stds_out, float* cov_out, icet_score* score_out);
icet_status icet_score_indexed(icet_ctx* ctx, const icet_params* p,
                               int32_t n_kf, const float* const* scan1, const int64_t* n1,
                               int32_t n_regs, const int32_t* kf_index, const float* const* scan2, const int64_t* n2,
                               const float* X, icet_score* score_out);
/* The best registration of every group, on the device.  group (HOST, n_regs): the group of registration r, 0 <= group[r] < n_groups, in any
 * order.  RULE: registration r is eligible when d_score[r].voxels >= max(1, ceil(0.5 x the largest voxels in its group)); among the eligible
 * the lowest chi2_per_voxel wins (NaN ranks last), ties go to the lowest r.  d_best (device, n_groups): the winner, or -1 for a group without
 * an eligible registration (an empty group included).  d_best_out (device, n_groups x 48, may be NULL): the winner's row of d_out (n_regs x 48,
 * may be NULL when d_best_out is), a zero row for -1.  Asynchronous on the context's stream; group is read before the call returns. */
icet_status icet_select_best_device(icet_ctx* ctx, int32_t n_regs, const int32_t* group, int32_t n_groups,
                                    const icet_score* d_score, const float* d_out, int32_t* d_best, float* d_best_out);

/* --- the keyframe store: keyframes built once and kept, whatever else runs on the context --------------------------------------------------
 * Loop-closure / relocalisation candidates: every k-th odometry frame's keyframe is put into a slot the caller chooses; a query registers and
 * scores a scan against any set of slots through the indexed kernels above, without rebuilding (or keeping the raw scans of) the candidates.
 * SHAPE.  create fixes the store's keyframe shape: bins_phi, bins_theta, n, thresh, buff and the keyframe-shaping flags ICET_FLAG_TRUE_SORT and
 *   ICET_FLAG_HALF_GAP_BOUNDS (runlen and the other flags are ignored).  capacity >= 1.  The store BORROWS ctx (device, stream, workspace), like a
 *   node: destroy the store before the context.  All slots start empty.  A grid above the 10 000-voxel limit: ICET_ERR_UNSUPPORTED; a failed
 *   allocation: ICET_ERR_NOMEM (*out is left NULL).  Device memory per slot: V x (48 + 80) + 2 x ((V + 1) & ~1) + 4 bytes (234 KB at 75 x 24,
 *   936 KB at 150 x 48).
 * PUT.  put_device builds the keyframes of n scans and parks keyframe k in slot slots[k] (HOST array of distinct entries, 0 <= slot < capacity).
 *   scan1 and d_rows (may be NULL) follow the rules of icet_keyframe_device_n.  A slot's tables are exactly what icet_keyframe_device_n builds for
 *   that scan in the store's shape, whatever batch the scan was put in.  A put replaces whatever the slot held; every other slot keeps its bytes.
 *   The store keeps no reference to the scan: its buffer may be reused once the put has run on the context's stream.  A put is a keyframe build on
 *   the context, so it un-parks the context's own keyframe (as icet_keyframe_device does); it never touches another store.  n == 0: ICET_OK,
 *   nothing.  Asynchronous on the context's stream; the host arrays are read before the call returns.
 * REGISTER / SCORE.  The three calls are icet_register_indexed_device, icet_register_indexed_scored_device and icet_score_indexed_device with
 *   kf_index replaced by slot_index (HOST array; every index must name an occupied slot; repeats and any order allowed).  p must match the store's
 *   shape (else ICET_ERR_BAD_ARG); ICET_FLAG_ROUNDTRIP_SCAN2, REJECT_MOVING, DOUBLE_W and TIMING apply per call; option "keep" on:
 *   ICET_ERR_UNSUPPORTED.  d_out / d_score carry exactly the bits icet_solve_batch_device / the indexed calls give for the expanded pair: the scan
 *   put into the slot (with its d_rows count), scan2[r] and x0[r].  These calls leave every slot and the context's parked keyframe as they were.
 * RESERVE.  reserve grows the store; every occupied slot keeps its bytes.  A smaller value: ICET_OK, nothing.  Synchronises the context's stream.
 * REFUSALS.  Every argument is checked before anything is touched; a refused call leaves every slot and the context's parked keyframe as they
 *   were.  ICET_ERR_BAD_ARG for a NULL store, n < 0, a slot out of range or empty, a slot named twice in one put, a bad scan descriptor, a shape
 *   mismatch. */
typedef struct icet_keyframe_store icet_keyframe_store;   /* opaque: slots of parked keyframe tables on one context's device */

icet_status icet_keyframe_store_create(icet_ctx* ctx, const icet_params* p, int32_t capacity, icet_keyframe_store** out);
icet_status icet_keyframe_store_destroy(icet_keyframe_store* s);
const char* icet_keyframe_store_last_error(const icet_keyframe_store* s);   /* never NULL; "null store" for NULL */
icet_status icet_keyframe_store_reserve(icet_keyframe_store* s, int32_t capacity);
icet_status icet_keyframe_store_put_device(icet_keyframe_store* s, int32_t n, const int32_t* slots,
                                           const icet_dev_scan* scan1, const int32_t* d_rows);
icet_status icet_keyframe_store_register_device(icet_keyframe_store* s, const icet_params* p, int32_t n_regs, const int32_t* slot_index,
                                                const icet_dev_scan* scan2, const float* d_x0, float* d_out);
icet_status icet_keyframe_store_register_scored_device(icet_keyframe_store* s, const icet_params* p, int32_t n_regs, const int32_t* slot_index,
                                                       const icet_dev_scan* scan2, const float* d_x0, float* d_out, icet_score* d_score);
icet_status icet_keyframe_store_score_device(icet_keyframe_store* s, const icet_params* p, int32_t n_regs, const int32_t* slot_index,
                                             const icet_dev_scan* scan2, const float* d_X, icet_score* d_score);
/* Test hook, like icet_debug_fetch: one OCCUPIED slot's tables on the host; synchronises the context's stream.  what = 0: n_slots (1 int32);
 * 1: the SlotHot records (12 words each: cluster_bounds row, mu1, voxel, 2 pad), count <= n_slots x 12; 2: the SlotFit records (20 words each:
 * mu1, sigma1 upper triangle / (n1_raw - 1), M = diag(l_diag) x evecs1 row-major, n1, voxel), count <= n_slots x 20; 3: slot_of_voxel (int16,
 * -1 = no slot), count <= V; 4: the slot's pose (16 float32, row-major 4 x 4; NaN entries when the slot has none), count <= 16; 5: its stamp (1 int64,
 * -1 without a pose), count <= 1; 6 / 7: the slot's appearance descriptor and weights ("loop closure by appearance" below). */
icet_status icet_keyframe_store_debug_fetch(icet_keyframe_store* s, int32_t slot, int32_t what, void* out, int64_t count);

/* --- loop closure against the store: find the candidates by pose, register, score, pick and gate in one call ---------------------------------
 * POSE.  A pose here is the PHYSICAL sensor pose in a world frame: 4 x 4 row-major float32 T = [R | t; 0 0 0 1], p_world = R p + t; R is taken as
 *   orthonormal.  It is NOT icet_node_result.pose: that member is the reference's chain X_homo = X_homo * [R(X) | t] (include/icet_nodes.h), while the
 *   solver's model is q = R(X)^T (p + t), i.e. the physical step of a registration result X is [R(X)^T | R(X)^T X_t].  For the small rotations of
 *   consecutive frames the two read alike; for a revisit with a real yaw difference the node's chain gives the yaw with the wrong sign.
 *   icet_pose_step_from_x writes that step; a caller chains T_world,k = T_world,k-1 * step.  A stamp is any int64 that orders the keyframes (a frame
 *   number, nanoseconds).
 * SET_POSE.  Gives n occupied, distinct slots a pose and a stamp (HOST arrays: n x 16 floats, n int64; read before the call returns).  In stream order
 *   with puts and queries.  A put into a slot clears that slot's pose; reserve carries poses and stamps over.  A slot without a pose is never a candidate,
 *   so a store that sets none behaves as before.
 * CANDIDATES.  For query q (pose poses[q], stamp stamps[q]; HOST arrays) slot j is eligible when it is occupied and has a pose,
 *   |stamps[q] - stamp_j| >= min_stamp_gap in 64-bit integers, and d2 <= fl(radius * radius) with d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)),
 *   dx = fl(t_q.x - t_j.x): float32, one rounding per operation; a NaN anywhere makes the slot ineligible.  The candidates are the first
 *   K = max_candidates eligible slots in ascending order of (d2, slot); d_cand (device, n_queries x K int32) gets them, -1 behind the last.
 *   d_x0_base (device, n_queries x K x 6, may be NULL): the start pose of each candidate, zeros for -1.
 * START POSE.  In double from the float32 poses, sums left to right: R_X = R_q^T R_j, X_t = R_q^T (t_q - t_j), theta = asin(clamp(R_X[2][0], -1, 1)),
 *   phi = atan2(-R_X[2][1], R_X[2][2]), psi = atan2(-R_X[1][0], R_X[0][0]); X0 = (X_t, phi, theta, psi), each value rounded to float32 once.
 *   Start s of a candidate is fl(X0 + start_offsets[s]) per component (HOST, n_starts x 6; NULL = zeros; by convention the first row is zero).
 * CLOSE.  Registration r = (q K + k) S + s: scan2[q] against candidate k of query q from start s, through the indexed kernels in scored mode (the bits
 *   of icet_keyframe_store_register_scored_device for the same slot, scan and X0); a missing candidate registers a scan of no rows.  The winner of
 *   query q is icet_select_best_device's over its K x S registrations; d_closure[q] (device) is its record.  accepted = slot >= 0 &&
 *   score.chi2_per_voxel <= max_chi2_per_voxel && score.voxels >= min_voxels.  d_cand (Q x K), d_x0 (Q K S x 6), d_out (Q K S x 48) and d_score (Q K S)
 *   may each be NULL (the store then uses buffers of its own).  1 <= n_queries <= 64, 1 <= K <= 32, 1 <= S <= 16.  Asynchronous on the context's stream.
 *   A store without an occupied slot: ICET_OK, every record has slot = -1 (d_out / d_score, when given, are zeroed).
 * The calls leave every slot, pose and the context's parked keyframe as they were.  Refusals as above (ICET_ERR_BAD_ARG: NULL store or array, a shape
 *   mismatch, K, S or n_queries out of range, a negative or NaN radius, an unoccupied or repeated slot in set_pose; ICET_ERR_UNSUPPORTED: option "keep"). */
typedef struct icet_closure_query {
    float   radius;               /* metres */
    int32_t max_candidates;       /* K */
    int64_t min_stamp_gap;        /* <= 0: none */
    int32_t n_starts;             /* S */
    float   max_chi2_per_voxel;   /* gate; +inf: none */
    int32_t min_voxels;           /* gate; 0: none */
    int32_t reserved;             /* zero */
} icet_closure_query;             /* 32 bytes */

typedef struct icet_closure {
    int32_t slot;                 /* the winner's slot, -1: none */
    int32_t reg;                  /* the winner's registration (q K + k) S + s, -1: none */
    int32_t accepted;             /* the gate */
    int32_t n_candidates;         /* eligible slots found, <= K */
    int64_t stamp;                /* the slot's stamp */
    float   d2;                   /* the slot's squared distance, as the candidate rule computed it */
    int32_t reserved0;            /* zero; the appearance query (below) puts the slot's column shift here, and its distance in d2 */
    float   x0[6];                /* the winner's start pose */
    int32_t reserved1[2];         /* zero; close_coarse_device (below) puts the winner's coarse score and shift word here */
    float   out[48];              /* the winner's row, layout of icet_solve_batch_device */
    icet_score score;             /* the winner's score */
} icet_closure;                   /* 288 bytes; without a winner x0, out and score are zero */

icet_status icet_keyframe_store_set_pose(icet_keyframe_store* s, int32_t n, const int32_t* slots, const float* poses, const int64_t* stamps);
icet_status icet_keyframe_store_candidates_device(icet_keyframe_store* s, int32_t n_queries, const float* poses, const int64_t* stamps,
                                                  const icet_closure_query* query, int32_t* d_cand, float* d_x0_base);
icet_status icet_keyframe_store_close_device(icet_keyframe_store* s, const icet_params* p, int32_t n_queries, const icet_dev_scan* scan2,
                                             const float* poses, const int64_t* stamps, const icet_closure_query* query, const float* start_offsets,
                                             icet_closure* d_closure, int32_t* d_cand, float* d_x0, float* d_out, icet_score* d_score);
/* One step of a pose chain from a registration result X (host; T: 16 floats).  T = [R(X)^T | R(X)^T X_t] in double, each entry rounded once. */
void icet_pose_step_from_x(const float X[6], float T[16]);

/* --- loop closure by appearance: find the candidates without poses ---------------------------------------------------------------------------
 * The pose search above needs the true revisit within `radius` of the live pose; after a long loop odometry has drifted further than that.  This
 * search compares what the scans look like: a rotation-invariant descriptor per keyframe, built on the device when the scan is put and kept beside
 * the slot, matched against a live scan's descriptor at every column shift.  The best shift is the yaw of the start pose.  No pose is read anywhere.
 * DESCRIPTOR.  rings x sectors bytes D[ring][sector] in the sensor frame.  A point (x, y, z), float32, one rounding per operation: rho = sqrt(fl(fl(x x) +
 *   fl(y y))); it counts when x, y, z are finite, rho^2 > 0 (exact-zero rows are skipped) and t = fl(rho kr) < rings; ring = floor(t); az = (float)atan2(
 *   (double)y, (double)x), sector = floor(fl(fl(az ka) + sectors / 2)), minus sectors when >= sectors, 0 when negative; height code q = 1 + floor(fl(fl(
 *   min(max(z, z_lo), z_hi) - z_lo) kz)) clamped to 1 .. 255.  kr = rings / rho_max, ka = sectors / 2 pi, kz = 254 / (z_hi - z_lo), each in double and
 *   rounded to float32 once.  D[ring][sector] is the largest q of the cell, 0 when empty.  Column weight w_j = (float)(1 / sqrt((double)sum_r D[r][j]^2)),
 *   0 for an empty column.  A maximum does not depend on order: the descriptor is bitwise reproducible whatever the batch.
 * DISTANCE of a live descriptor (Dq, wq) to a slot's (Dc, wc) at shift s, j' = (j + s) mod sectors: G_j = sum_r Dq[r][j] Dc[r][j'] (an integer),
 *   c_j = fl(fl((float)G_j wq_j) wc_j'); column j is valid when both weights are positive, m their number; m < ceil(sectors / 4): d_s = +inf; else
 *   d_s = (float)(1 - (sum of (double)c_j over the valid j, ascending) / m), a negative value becoming +0.  The slot's distance is the smallest d_s, ties to
 *   the lowest s: the slot's shift.
 * ENABLE.  enable_appearance allocates the descriptor table -- capacity x (4 ceil(rings / 4) sectors + 4 sectors + 4) bytes, 2.9 KB per slot at the
 *   defaults -- and fixes the parameters (NULL: sectors 120, rings 20, rho_max 80, z_lo -3, z_hi 12).  Once per store (again: ICET_ERR_BAD_ARG); sectors
 *   even, 8 .. 360; rings 1 .. 64; rho_max > 0; z_hi > z_lo; reserved words zero; else ICET_ERR_BAD_ARG.  Slots put BEFORE it have no descriptor and are never
 *   appearance candidates.  From then on put_device also builds the descriptor of every scan it parks, in stream order behind the park, honouring d_rows; a
 *   put replaces the slot's descriptor and clears its stamp; the slot's keyframe tables are the bytes they would be without.  reserve carries descriptors over.
 *   A store that never enables appearance issues exactly the launches it did.  Synchronises the context's stream.
 * DESCRIBE.  describe_device writes the descriptors of n device scans (rules of icet_keyframe_device_n for scan and d_rows): d_desc n x rings x sectors
 *   bytes, d_weight n x sectors floats (device).  Asynchronous.  debug_fetch what = 6: a slot's descriptor bytes (count <= rings x sectors), 7: its weights
 *   (count <= sectors); a slot without a descriptor: ICET_ERR_BAD_ARG.
 * SET_STAMP.  Gives n occupied, distinct slots a stamp (HOST arrays) without a pose, so that min_stamp_gap can keep the frames just behind the vehicle from
 *   being "revisits".  In stream order; a put clears the stamp (to -1), as it does now.
 * CANDIDATES.  Slot j is eligible for query q when it is occupied, has a descriptor, |stamps[q] - stamp_j| >= min_stamp_gap (when > 0; stamps may be NULL
 *   when it is <= 0) and d <= max_distance, which is READ FROM THE `radius` MEMBER of icet_closure_query (a NaN distance fails).  The candidates are the first
 *   K eligible slots in ascending (d, slot); d_cand (device, Q x K) gets them, -1 behind the last; d_dist (Q x K floats, may be NULL) their distances, +inf
 *   for -1; d_shift (Q x K int32, may be NULL) their shifts, -1 for -1; d_x0_base (Q x K x 6, may be NULL) their start poses, zeros for -1.
 * START POSE.  a = (double)s (2 pi / sectors), minus 2 pi when above pi; X0 = (0, 0, 0, 0, 0, (float)a): psi of R(X0) = R_q^T R_j, live sector j being keyframe
 *   sector j + s.  Start i is fl(X0 + start_offsets[i]).  The translation is NOT found: give a lattice of offsets (INTEGRATION, "Loop closure without poses").
 * CLOSE.  close_appearance_device is close_device without poses: descriptors of the Q scans, search, resolve, the indexed registrations r = (q K + k) S + s in
 *   scored mode, icet_select_best_device's winner per query, the gate, one icet_closure record per query, in which d2 carries the appearance distance and
 *   reserved0 the shift.  Limits, optional buffers and refusals are those of close_device, plus ICET_ERR_BAD_ARG when appearance is not enabled.
 * Every argument is checked before anything is touched.  Asynchronous on the context's stream (the host arrays are read before the call returns); never
 *   captured into a graph.  The queries leave every slot, descriptor, pose, stamp and the context's parked keyframe as they were. */
typedef struct icet_appearance_params {
    int32_t sectors;              /* A: even, 8 .. 360 */
    int32_t rings;                /* 1 .. 64 */
    float   rho_max;              /* metres, > 0 */
    float   z_lo, z_hi;           /* metres in the sensor frame, z_hi > z_lo */
    int32_t reserved[3];          /* zero */
} icet_appearance_params;         /* 32 bytes */

icet_status icet_keyframe_store_enable_appearance(icet_keyframe_store* s, const icet_appearance_params* ap);
icet_status icet_keyframe_store_describe_device(icet_keyframe_store* s, int32_t n, const icet_dev_scan* scan, const int32_t* d_rows,
                                                uint8_t* d_desc, float* d_weight);
icet_status icet_keyframe_store_set_stamp(icet_keyframe_store* s, int32_t n, const int32_t* slots, const int64_t* stamps);
icet_status icet_keyframe_store_candidates_appearance_device(icet_keyframe_store* s, int32_t n_queries, const icet_dev_scan* scan2, const int64_t* stamps,
                                                             const icet_closure_query* query, int32_t* d_cand, float* d_dist, int32_t* d_shift,
                                                             float* d_x0_base);
icet_status icet_keyframe_store_close_appearance_device(icet_keyframe_store* s, const icet_params* p, int32_t n_queries, const icet_dev_scan* scan2,
                                                        const int64_t* stamps, const icet_closure_query* query, const float* start_offsets,
                                                        icet_closure* d_closure, int32_t* d_cand, float* d_x0, float* d_out, icet_score* d_score);

/* --- coarse alignment: find a closure's start translation (and settle a half turn) by grid correlation -----------------------------------------
 * Both searches above hand the registration a start pose that is often outside the solver's basin: the appearance search finds the yaw and not the
 * translation, the pose search inherits the drift of two poses.  This search is coarse, exhaustive and all integers: a bird's-eye bit grid of the live scan's
 * vertical structure is correlated against the same grid kept beside each slot, over a window of cell shifts and a few yaw hypotheses.
 * CELL of (x, y), float32, one rounding per operation: u = fl(fl(x kc) + G / 2); the coordinate is inside when u >= 0 && u < G (a NaN is outside), ix =
 *   floor(u); likewise iy from y.  kc = 1 / cell, kz = 254 / (z_hi - z_lo): in double, rounded to float32 once; span_codes = ceil(min_span (254 / (z_hi - z_lo)))
 *   in double from the float32 parameters.
 * STRUCTURE POINTS of a scan, decided in the sensor frame once per scan: a point counts when x, y, z are finite, fl(fl(x x) + fl(y y)) > 0 (exact-zero rows are
 *   skipped) and its cell is inside; its height code is q = floor(fl(fl(min(max(z, z_lo), z_hi) - z_lo) kz)).  A cell SPANS when the largest minus the
 *   smallest q of its counting points is >= span_codes (flat ground does not, whatever the sensor height).  A counting point whose cell spans is a structure
 *   point.  Minima and maxima do not depend on order.
 * GRID of a scan under a transform: the cells its structure points hit after the transform; G rows (ix) of G / 32 words, bit iy & 31 of word iy >> 5 (8 KB at
 *   the defaults).  A keyframe's grid uses the identity: it is exactly its spanning cells.
 * HYPOTHESIS h of a live scan with base start pose X0 (six float32): delta_h = (double)y yaw_step + f pi, y = -Y .. Y, f = 0 / 1 (1 only with half_turn),
 *   h = f (2 Y + 1) + (y + Y).  R_h = R(X0) Rz(delta_h) in double, Rz(delta) the solver's R(0, 0, delta), sums left to right; M = R_h^T, each entry rounded to
 *   float32 once; u = fl(p + X0_t) per component; x' = fl(fl(fl(M00 ux) + fl(M01 uy)) + fl(M02 uz)), y' likewise with row 1.
 * SCORE S_h(a, b), |a|, |b| <= window: the number of live cells (i, j) whose slot cell (i + a, j + b) is set; cells shifted off the grid are dropped.
 * WINNER: largest S; then smallest a a + b b; then smallest h; then smallest a; then smallest b -- one 64-bit key (S << 32 | 4095 - (a a + b b) << 20 | 63 - h << 14 |
 *   32 - a << 7 | 32 - b) whose maximum does not depend on the launch shape.  found = 1 when the slot has a grid and the best S >= min_score; else the start
 *   stays X0.
 * START POSE of the winner: d = ((double)a cell, (double)b cell, 0); R(X) = R_h, X_t = X0_t + R_h d, in double, sums left to right; the angles by the inverse
 *   of the pose search's rule, -pi becoming pi; each of the six values rounded to float32 once.  (q = R_h^T (p + X0_t) + d = R(X)^T (p + X_t).)  Where nothing
 *   moves the value is X0's own, bit for bit: the translation when a = b = 0, the angles when y = 0 and f = 0.
 * ENABLE.  enable_coarse allocates the grid table -- capacity x (G G / 8 + 4) bytes -- and fixes the parameters (NULL: cells 256, cell 0.25, z_lo -3, z_hi 12,
 *   min_span 0.5).  Once per store (again: ICET_ERR_BAD_ARG); cells a multiple of 32, 64 .. 512; cell > 0; z_hi > z_lo; min_span > 0; reserved words zero; else
 *   ICET_ERR_BAD_ARG.  Independent of enable_appearance.  Slots put BEFORE it have no grid: the search reports found = 0 for them.  From then on put_device also
 *   builds the grid of every scan it parks, in stream order behind the park, honouring d_rows; a put replaces exactly its own slot's grid; reserve carries the
 *   grids over.  A store that never enables it issues exactly the launches it did.  Synchronises the context's stream.
 * GRID.  coarse_grid_device writes the grids of n device scans under the identity (rules of describe_device for scan and d_rows): d_grid n x G x G / 32 words
 *   (device).  Asynchronous.  debug_fetch what = 8: a slot's grid (count <= G G / 32 words); a slot without one: ICET_ERR_BAD_ARG.
 * ALIGN.  coarse_align_device searches Q x K candidates: d_cand (device, Q x K slots, -1: none) and d_x0_base (device, Q x K x 6) as either candidates call
 *   writes them, or the caller's own.  d_x0_out (Q x K x 6, may be NULL) gets the start poses -- X0 where found = 0, zeros for a candidate of -1 --, d_match
 *   (Q x K records, may be NULL) the winners: score, a, b, h and the bit counts of the winning live grid and of the slot's grid whenever the slot has a grid,
 *   zeros otherwise.  1 <= Q <= 64, 1 <= K <= 32, window 0 .. 32, n_yaw 0 .. 8, min_score >= 1, reserved words zero.
 * CLOSE.  close_coarse_device is close_device (poses given) or close_appearance_device (poses NULL: candidates by appearance, which must be enabled) with
 *   the coarse alignment of each candidate's base start in between: registrations r = (q K + k) S + s in scored mode from fl(X0_coarse + start_offsets[s]),
 *   icet_select_best_device's winner, the gate, one icet_closure record per query, filled as those calls fill it; in addition reserved1[0] carries the winner's
 *   coarse score and reserved1[1] h | (a + 32) << 8 | (b + 32) << 16.  d_match (Q x K, may be NULL) as above.  Limits, optional buffers and refusals are those of
 *   close_device, plus ICET_ERR_BAD_ARG when coarse alignment is not enabled.
 * Every argument is checked before anything is touched.  Asynchronous on the context's stream (the host arrays are read before the call returns); never
 *   captured into a graph.  The calls leave every slot, grid, descriptor, pose, stamp and the context's parked keyframe as they were. */
typedef struct icet_coarse_params {
    int32_t cells;                /* G: a multiple of 32, 64 .. 512 */
    float   cell;                 /* metres, > 0 */
    float   z_lo, z_hi;           /* metres in the sensor frame, z_hi > z_lo */
    float   min_span;             /* metres, > 0 */
    int32_t reserved[3];          /* zero */
} icet_coarse_params;             /* 32 bytes */

typedef struct icet_coarse_search {
    int32_t window;               /* M_w: shifts -window .. window cells in x and y, 0 .. 32 */
    int32_t n_yaw;                /* Y: yaw hypotheses -Y .. Y steps, 0 .. 8 */
    float   yaw_step;             /* radians */
    int32_t half_turn;            /* 0 / 1: every yaw hypothesis also turned by pi */
    int32_t min_score;            /* >= 1 */
    int32_t reserved[3];          /* zero */
} icet_coarse_search;             /* 32 bytes */

typedef struct icet_coarse_match {
    int32_t score;                /* S of the winner */
    int32_t a, b;                 /* its shift in cells */
    int32_t h;                    /* its hypothesis */
    int32_t live_bits;            /* bits of the winning live grid */
    int32_t key_bits;             /* bits of the slot's grid */
    int32_t found;                /* 1: score >= min_score, the start pose moved */
    int32_t reserved;             /* zero */
} icet_coarse_match;              /* 32 bytes */

icet_status icet_keyframe_store_enable_coarse(icet_keyframe_store* s, const icet_coarse_params* cp);
icet_status icet_keyframe_store_coarse_grid_device(icet_keyframe_store* s, int32_t n, const icet_dev_scan* scan, const int32_t* d_rows, uint32_t* d_grid);
icet_status icet_keyframe_store_coarse_align_device(icet_keyframe_store* s, int32_t n_queries, const icet_dev_scan* scan2, const int32_t* d_rows, int32_t K,
                                                    const int32_t* d_cand, const float* d_x0_base, const icet_coarse_search* search, float* d_x0_out,
                                                    icet_coarse_match* d_match);
icet_status icet_keyframe_store_close_coarse_device(icet_keyframe_store* s, const icet_params* p, int32_t n_queries, const icet_dev_scan* scan2,
                                                    const float* poses, const int64_t* stamps, const icet_closure_query* query,
                                                    const icet_coarse_search* search, const float* start_offsets, icet_closure* d_closure, int32_t* d_cand,
                                                    float* d_x0, float* d_out, icet_score* d_score, icet_coarse_match* d_match);

/* --- snapshots: a store to a file and back, bit for bit ------------------------------------------------------------------------------------------
 * A store keeps no raw scans, so a map made in one process is carried to another as a file: the occupied slots at their used length (n_slots records, not V),
 * their poses and stamps, and their descriptors and grids where the store has them.  The format -- little-endian, every section 16-byte aligned, every byte
 * under a checksum, reserved bytes and padding zero -- and its validation are icet_amd/csrc/icet_snapshot.h.
 * SAVE.  In stream order behind whatever was enqueued.  slots: n distinct occupied slots (HOST array), or NULL for every occupied slot (n is then ignored);
 *   else ICET_ERR_BAD_ARG.  The payload moves in chunks of option "snapshot_chunk_bytes" (icet_set_option on the store's context; default and 0: 64 MiB; never
 *   less than the largest single slot; the file does not depend on it): packed on the device, copied into one of two pinned buffers and written while the next
 *   chunk packs.  Written to path + ".tmp" and renamed on success: a failed save leaves nothing at `path`.  Returns after the file is closed.  A path that
 *   cannot be written: ICET_ERR_BAD_ARG, the reason in last_error.
 * LOAD.  Reads and validates the whole file on the host (every checksum, every offset and size, and the contents a kernel would index by), then holds it
 *   against the store: the keyframe shape (grid, n, bit patterns of thresh and buff, the two keyframe-shaping flags) must be equal and every slot + slot_offset a
 *   slot of the store (reserve first; snapshot_info gives the highest slot).  A file that carries descriptors loads into a store with appearance enabled only
 *   when the parameters are bit-equal; into a store without, the descriptors are skipped; a file without them gives slots that have none and are never
 *   appearance candidates, like slots put before enable_appearance.  Grids likewise.  Any failure of these: ICET_ERR_BAD_ARG, the reason in last_error, and
 *   nothing is touched.  Only then are the chunks uploaded and unpacked.  A loaded slot replaces everything the target slot held -- tables, pose and stamp,
 *   descriptor and grid, each cleared where the entry has none --; every other slot keeps its bytes.  Synchronises the stream before it returns.  The tables do
 *   not move: a replayed graph reads the new bytes as it does after a put.
 * INFO / SLOTS.  Host only, no store: the validated file's header, and its slots with their stamps in ascending order (at most cap are written, *n_out is the
 *   file's count; stamps may be NULL).  A file that cannot be read or is refused: ICET_ERR_BAD_ARG.
 * With option "keep" on, save and load answer ICET_ERR_UNSUPPORTED, as the store's other calls do.  Neither touches the context's parked keyframe. */
typedef struct icet_snapshot_info {
    icet_params shape;            /* runlen 0; flags: the keyframe-shaping flags */
    int32_t V;                    /* bins_phi * bins_theta */
    int32_t entries;              /* saved slots */
    int32_t highest_slot;         /* -1 when there is none */
    int32_t has_appearance, has_coarse;      /* 1: the block below holds the saved store's parameters */
    icet_appearance_params appearance;
    icet_coarse_params coarse;
    int64_t file_bytes;
} icet_snapshot_info;             /* 120 bytes */

icet_status icet_keyframe_store_save(icet_keyframe_store* s, const char* path, int32_t n, const int32_t* slots);
icet_status icet_keyframe_store_load(icet_keyframe_store* s, const char* path, int32_t slot_offset);
icet_status icet_keyframe_store_snapshot_info(const char* path, icet_snapshot_info* info);
icet_status icet_keyframe_store_snapshot_slots(const char* path, int32_t cap, int32_t* slots, int64_t* stamps, int32_t* n_out);

/* Pre-size the workspace (so the first timed call does not allocate). */
icet_status icet_reserve(icet_ctx* ctx, const icet_params* p, int32_t n_pairs, int64_t total_n1, int64_t total_n2);

/* Wall-clock-free device timing of the most recent icet_solve_batch_device call, measured with HIP
 * events on the context's stream: [0] keyframe build ms, [1] Gauss-Newton loop ms, [2] ms inside the
 * bin/accumulate kernel only (sum over iterations; -1 unless ICET_FLAG_TIMING was set), [3] number of
 * accumulate launches timed. */
icet_status icet_last_timing(icet_ctx* ctx, float out_ms[4]);
/* The same call's point-pass launches one by one (ICET_FLAG_TIMING): acc_ms[it] = HIP-event time of iteration it's launch, *n_out = how many were written (<= cap). */
icet_status icet_last_timing_iters(icet_ctx* ctx, float* acc_ms, int32_t cap, int32_t* n_out);
/* The keep list of the point pass after the most recent throughput batch (option "keep"): out[4 k ..] = { mode at the end, groups of 4 points in pair k's last list,
 * passes that walked a list, lists built }.  ICET_ERR_BAD_ARG when the last call did not use the keep list (small batch, option off). */
icet_status icet_keep_stats(icet_ctx* ctx, int32_t n_pairs, int32_t* out);

/* Diagnostic hook for the parity tests: copy an internal per-point array of the scan-1 (keyframe) build
 * of the most recent call to the host.  `what`: 0 = float32 r of scan 1 in input order
 * (utils::cartesianToSpherical, src/utils.cpp:99,116); 1 = uint16 per row: bits 0-13 the row's voxel
 * bins_theta * binPhi + binTheta (sortSphericalCoordinates, src/icet.cpp:545-549), bit 14 "classified with
 * the literal formulas", bit 15 "r is exactly 0" (theta / phi themselves are not materialised: only decisions and the
 * Gaussians need them); 3 = int32 src[v], the original row that
 * sits at position v after the reference's sort + swap loop (src/icet.cpp:72-83); 4 = int32 per-pair
 * flags (bit 0: the bounded parallel walk overflowed and the serial replay was used); 6 = ONE int32: 1 if this device passed the
 * context's LDS-atomic order self-test (option "lds_rank").  `count` elements
 * from the start of the batch's concatenated scan-1 arrays (pairs for what = 4). */
icet_status icet_debug_fetch(icet_ctx* ctx, int32_t what, void* out, int64_t count);

/* Diagnostic hook for the parity tests: the 6x6 tail of one Gauss-Newton iteration (noise_mat = pinv(HTWH), pred_stds, checkCondition, dx:
 * src/icet.cpp:410-433) evaluated on the device for n host-side matrices, through the same device function the solve kernel runs.
 * htwh: n x 36 row-major, htwdz: n x 6; out: n x 56 = cov[36] | pred_stds[6] | dx[6] | eigenvalues[6] (NaN on the Cholesky route) |
 * pruned axes | route (0 Cholesky inverse, 2 literal restatement; option "gn_cond_bound"). */
icet_status icet_debug_gn_tail(icet_ctx* ctx, const float* htwh, const float* htwdz, int32_t n, float* out);
/* Diagnostic hook for the parity tests: the per-voxel weight W = pinv(.) of ICET_FLAG_REFERENCE_W (Eigen's float CompleteOrthogonalDecomposition, src/icet.cpp:320-321) for n
 * host-side 3 x 3 matrices (row-major, n x 9 in, n x 9 out), through the device function the solve kernel runs. */
icet_status icet_debug_pinv3(icet_ctx* ctx, const float* a, int32_t n, float* out);
/* Diagnostic hook for the parity tests: the per-voxel weight W = pinv(.) of ICET_FLAG_DOUBLE_W (the double-precision pseudo-inverse with the 3 eps rank rule) for n
 * host-side symmetric 3 x 3 matrices, packed (xx, xy, xz, yy, yz, zz): n x 6 in, n x 6 out, through the device function the solve kernel runs. */
icet_status icet_debug_pinv3_double(icet_ctx* ctx, const float* a, int32_t n, float* out);
/* Diagnostic hook for the point-pass tests: the arguments and the ONE point pass of icet_score_indexed_device (scan 2 r at pose d_X[r] against parked keyframe
 * kf_index[r]), then, instead of the score, every voxel's raw accumulator record as the point pass and the drain of its overflow list leave it:
 * d_sums (device, 16-byte aligned -- ICET_ERR_BAD_ARG otherwise --, n_regs * V * 80 bytes) = n_regs x V records of 80 bytes, indexed by voxel id (V = bins_phi * bins_theta, voxel = bins_theta * polar bin + azimuth bin):
 *     uint32 n2 (points in the voxel's angular bin), uint32 m (those inside the cluster bounds), then nine int64 = round(s * 2^36) summed over flushes for
 *     s = sum dx, dy, dz, dx dx, dx dy, dx dz, dy dy, dy dz, dz dz of d = q - mu1 over the m points; zeros for a voxel that is not active in the keyframe.
 * The accumulators and the overflow count are left at zero, as a solve leaves them.  Never captured into a graph. */
icet_status icet_debug_point_sums_device(icet_ctx* ctx, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2,
                                         const float* d_X, void* d_sums);
/* Diagnostic hook for the per-voxel algebra tests: the arguments of icet_debug_point_sums_device and the same ONE point pass at the poses d_X; the records are copied to
 * d_sums (same layout and alignment rule) but LEFT IN PLACE, and the production solve kernel of Gauss-Newton iteration p->runlen - 1 (>= 0; the index places the
 * moving-voxel gate of ICET_FLAG_REJECT_MOVING) then consumes exactly those records.  Device outputs: d_xf n_regs x 48 floats, the transform record the kernels read
 * (t[3] | R[9] row-major | angles[3] | pad | J[27]); d_htwh n_regs x 36 and d_htwdz n_regs x 6, H^T W H and H^T W dz as that kernel formed them; d_out n_regs x 48, the
 * iteration's X | pred_stds | cov.  The call returns after the stream has drained; the workspace is left as every solve leaves it.  Never captured into a graph. */
icet_status icet_debug_gn_terms_device(icet_ctx* ctx, const icet_params* p, int32_t n_regs, const int32_t* kf_index, const icet_dev_scan* scan2,
                                       const float* d_X, void* d_sums, float* d_xf, float* d_htwh, float* d_htwdz, float* d_out);
/* Diagnostic hook for the point-pass tests: n host-side floats through the float -> 2^36 fixed-point conversions of the point pass; out: n x 3 uint64 =
 * the two-instruction biased form (defined for |v| < 2^15) | the wide biased form | the unbiased form that selects between them per value. */
icet_status icet_debug_fix(icet_ctx* ctx, const float* v, int32_t n, uint64_t* out);
/* Diagnostic hook for the shared arithmetic rule: n host-side rows x[n] | y[n] | z[n] (leading dimension ld >= n) through the device functions
 * every kernel takes its angles and round trips from.  out: 12 columns of n 32-bit words -- r | theta | phi of cartesianToSpherical, the voxel of (theta, phi) on a
 * T x P grid (int32), x | y | z of the round trip of ANY row (what ICET_FLAG_ROUNDTRIP_SCAN2 stores), and theta | phi | x | y | z of the ordinary-row round trip that
 * the scan-1 fit runs (NaN for rows whose r is 0, infinite or NaN).  Drains the stream before it returns. */
icet_status icet_debug_spherical(icet_ctx* ctx, const float* xyz, int32_t n, int32_t ld, int32_t T, int32_t P, float* out);

/* --- pose-graph optimisation: corrected poses from closure records --------------------------------------------------------
 * GRAPH.  n poses (float32 4 x 4 row-major, the store's POSE convention), one odometry edge (k, k + 1) per k < n - 1 and n_closures closure edges
 *   (ci[c], cj[c]), ci != cj, otherwise free: repeats, adjacent and reversed pairs, ends on fixed nodes.  Edge e < n - 1 is the odometry edge, edge
 *   n - 1 + c is closure c.  An edge (i, j) carries a measurement X (six float32: what a registration of live scan j against keyframe i returns -- the START
 *   POSE rule above, in double and unrounded: R_X = R_j^T R_i, X_t = R_j^T (t_j - t_i), the angles of R_X) and a 6 x 6 float32 information matrix, used as
 *   0.5 (m + m^T) in double.  Node 0 and every node with fixed[k] != 0 do not move.
 * OPTIMISE.  Gauss-Newton in double on chi2 = sum e^T Omega e, e = predicted - X with the angles wrapped to (-pi, pi]; right updates T <- T Exp(dx); central
 *   differences of step 1e-6.  Per iteration: the edges are linearised, H = sum J^T Omega J and g = sum J^T Omega e are assembled per node in the order of its
 *   incidence list (no atomics), and H dx = -g is solved by conjugate gradients preconditioned with the block-tridiagonal part of H (every diagonal block, every
 *   coupling of neighbouring nodes) through the block Cholesky factorisation below: one factorisation per iteration, one band solve per CG iteration, stop at
 *   sqrt(r.z / r0.z0) <= pcg_tol or after max_pcg band solves (0: 12 x the closures off the band + 8; a graph with none takes exactly one).  `damping` is added to
 *   the diagonal of H.  A step that does not lower chi2 is undone and ends the run: ICET_POSE_GRAPH_CONVERGED when max |dx| < dx_tol, else _STALLED; a step
 *   that does is kept, and max |dx| < dx_tol then ends the run _CONVERGED; gn_iters iterations without either: _ITERATION_CAP.
 * FAILURE.  A band pivot at or below 1e-13 of its diagonal entry (or p.Hp <= 0 in CG): _NOT_POSITIVE_DEFINITE; a chi2, pivot or r.z that is not finite:
 *   _NON_FINITE.  The outputs are then the inputs: poses_out the input bits, poses64_out their doubles, chi2_final = chi2_initial, both rows of edge_chi2 the
 *   initial values.  The status is a RESULT: the call returns ICET_OK.
 * OUTPUT.  poses_out n x 16 float32: every pose rounded once, row 3 = (0, 0, 0, 1); a fixed node returns its input bits.  poses64_out (may be NULL) n x 12
 *   doubles, R row-major then t.  edge_chi2 (may be NULL) 2 x E doubles, E = n - 1 + n_closures: chi2 per edge at the start | at the end.  gn_iterations counts
 *   the linearisations, pcg_iterations the band solves.  Same inputs, same bits, run to run.
 * The first form takes HOST arrays.  In the _device form poses, odo_X, odo_info, clo_X, clo_info, poses_out, poses64_out and edge_chi2 are DEVICE pointers (8-byte
 * aligned doubles); ci, cj, fixed, opt and result stay on the host.  Both synchronise: they return when the result is known.  The context's parked keyframe and
 * workspace are not touched.  ICET_ERR_BAD_ARG: a NULL ctx, poses, poses_out or result; odo_X / odo_info NULL with n > 1; ci, cj, clo_X or clo_info NULL with
 * n_closures > 0; n < 1 or > 4096; n_closures < 0 or > 512; a closure index out of range or ci[c] == cj[c]; gn_iters < 1. */
#define ICET_POSE_GRAPH_CONVERGED 0
#define ICET_POSE_GRAPH_ITERATION_CAP 1
#define ICET_POSE_GRAPH_NOT_POSITIVE_DEFINITE 2
#define ICET_POSE_GRAPH_NON_FINITE 3
#define ICET_POSE_GRAPH_STALLED 4
typedef struct icet_pose_graph_options {
    int32_t gn_iters;             /* >= 1 */
    int32_t max_pcg;              /* band solves per Gauss-Newton iteration; 0 = 12 x closures off the band + 8 */
    double  dx_tol, damping;
    double  pcg_tol;              /* <= 0: the default, 1e-10 */
} icet_pose_graph_options;        /* 32 bytes; NULL = 10, 0, 1e-7, 0, default */
typedef struct icet_pose_graph_result {
    double  chi2_initial, chi2_final, max_dx;
    int32_t status, gn_iterations, pcg_iterations;
    int32_t solver;               /* 0: conjugate gradients ran, 1: the direct solve (option "pg_solver", below) */
} icet_pose_graph_result;         /* 40 bytes */
icet_status icet_pose_graph_optimize(icet_ctx* ctx, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                     const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                     const icet_pose_graph_options* opt, float* poses_out, double* poses64_out, double* edge_chi2, icet_pose_graph_result* result);
icet_status icet_pose_graph_optimize_device(icet_ctx* ctx, int32_t n, const float* d_poses, const float* d_odo_X, const float* d_odo_info, int32_t n_closures,
                                            const int32_t* ci, const int32_t* cj, const float* d_clo_X, const float* d_clo_info, const uint8_t* fixed,
                                            const icet_pose_graph_options* opt, float* d_poses_out, double* d_poses64_out, double* d_edge_chi2,
                                            icet_pose_graph_result* result);
/* ROBUST KERNELS: the same optimiser by iteratively reweighted least squares, so that a wrong closure cannot bend the map.  Per edge s = e^T Omega e and a
 * threshold c > 0 in chi2 units (`scale`; ICET_PG_ROBUST_DEFAULT_SCALE is the 99 % quantile of chi2 with six degrees of freedom):
 *   kind 0 none            rho = s                                   w = 1
 *   kind 1 Huber           rho = s (s <= c), 2 sqrt(c s) - c         w = 1 (s <= c), sqrt(c / s)
 *   kind 2 Cauchy          rho = c log1p(s / c)                      w = 1 / (1 + s / c)
 *   kind 3 Geman-McClure   rho = c s / (c + s)                       w = (c / (c + s))^2
 * (where s is not above zero: rho = s, w = 1).  The objective is F = sum rho(s_e).  The closures take the kind; the odometry edges only with flag
 * ICET_PG_ROBUST_ODOMETRY.  Per iteration the weights w_e at the current poses scale the edges: H = sum w_e J^T Omega J (+ damping), g = sum w_e J^T Omega e;
 * the step is kept only if F falls.  Statuses, failures, fixed nodes, the float32 rounding and the linear solves (option "pg_solver") are
 * icet_pose_graph_optimize's.  The arguments are its arguments with `robust` (NULL: kind 0) behind opt and edge_weight (E doubles, may be NULL; a DEVICE
 * pointer in the _device form) behind edge_chi2: every edge's w at the chi2 of the returned poses, 1 for an edge the flags leave alone.
 * result: base.chi2_initial and base.chi2_final are the RAW sums of chi2, cost_initial and cost_final are F, downweighted counts the edges whose final w is
 * below 0.5.  After a failure (status 2 or 3) the outputs are the inputs, edge_weight is w at the start's chi2 and cost_final = cost_initial.  With kind 0 the
 * run is icet_pose_graph_optimize's, bit for bit, every weight 1 and cost = chi2.  ICET_ERR_BAD_ARG as icet_pose_graph_optimize, and: a kind outside 0 .. 3,
 * a flag bit other than bit 0, with a kind a scale that is not finite and positive. */
#define ICET_PG_ROBUST_NONE 0
#define ICET_PG_ROBUST_HUBER 1
#define ICET_PG_ROBUST_CAUCHY 2
#define ICET_PG_ROBUST_GEMAN_MCCLURE 3
#define ICET_PG_ROBUST_ODOMETRY 1
#define ICET_PG_ROBUST_DEFAULT_SCALE 16.8119
typedef struct icet_pose_graph_robust {
    int32_t kind, flags;
    double  scale;
} icet_pose_graph_robust;         /* 16 bytes; NULL = kind 0 */
typedef struct icet_pose_graph_robust_result {
    icet_pose_graph_result base;
    double  cost_initial, cost_final;
    int32_t downweighted;
    int32_t reserved;             /* zero */
} icet_pose_graph_robust_result;  /* 64 bytes */
icet_status icet_pose_graph_optimize_robust(icet_ctx* ctx, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                            const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                            const icet_pose_graph_options* opt, const icet_pose_graph_robust* robust, float* poses_out, double* poses64_out,
                                            double* edge_chi2, double* edge_weight, icet_pose_graph_robust_result* result);
icet_status icet_pose_graph_optimize_robust_device(icet_ctx* ctx, int32_t n, const float* d_poses, const float* d_odo_X, const float* d_odo_info,
                                                   int32_t n_closures, const int32_t* ci, const int32_t* cj, const float* d_clo_X, const float* d_clo_info,
                                                   const uint8_t* fixed, const icet_pose_graph_options* opt, const icet_pose_graph_robust* robust,
                                                   float* d_poses_out, double* d_poses64_out, double* d_edge_chi2, double* d_edge_weight,
                                                   icet_pose_graph_robust_result* result);
/* Test hook: the optimiser's FIRST Gauss-Newton iteration with every intermediate array copied out.  The arguments of icet_pose_graph_optimize (HOST arrays;
 * opt's gn_iters and dx_tol are not used), then K >= 0 vectors p (K x n x 6 doubles, may be NULL with K = 0).  On the context's stream, the production
 * kernels in the production order: the start's residuals and chi2, one linearisation, the assembly of the band and the off-band blocks, the band's
 * factorisation, the conjugate-gradient loop of the optimiser itself, the trial poses T Exp(x) and their chi2; then q = H p per caller vector through the
 * kernel the loop uses.  Every array of *out is a HOST pointer the caller sizes, or NULL to skip it:
 *   J E x 72 (6 x 12 per edge: node i's six columns, then node j's) | res E x 6 and chi_start E (at the start) | chi_trial E | D, B n x 36 (B[k]: the block at
 *   (k, k - 1)) | A n_closures x 36 (the block at (ci, cj); zeros for a closure on the band or with a fixed end) | g, x n x 6 | Pt n x 12 | q K x n x 6 |
 *   cg_scalars 2 x cg_capacity: per band solve its r.z, then the p.Hp of the step that followed (NaN where none did); band_solves pairs are written.
 * factor_status / cg_status: 0 or an ICET_POSE_GRAPH_* failure; cg_end: how the loop ended (ICET_PG_CG_*); cap: the band solves it was allowed; trial: 1 when
 * the trial poses were taken (the optimiser stops before them on a failure, and before the linearisation on a start chi2 that is not finite).  Synchronises. */
#define ICET_PG_CG_TOLERANCE 0
#define ICET_PG_CG_ZERO 1
#define ICET_PG_CG_CAP 2
#define ICET_PG_CG_FAILED 3
typedef struct icet_pose_graph_step {
    double *J, *res, *chi_start, *chi_trial, *D, *B, *A, *g, *x, *Pt, *q, *cg_scalars;
    int32_t cg_capacity;          /* in: pairs cg_scalars has room for */
    int32_t factor_status, cg_status, band_solves, cg_end, cap, c_offband, trial;
    double  chi2_start, chi2_trial, max_dx;
} icet_pose_graph_step;           /* 152 bytes */
icet_status icet_debug_pose_graph_step(icet_ctx* ctx, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                       const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                       const icet_pose_graph_options* opt, int32_t K, const double* p, icet_pose_graph_step* out);
/* THE DIRECT SOLVE (option "pg_solver" of icet_set_option: 0 conjugate gradients, the default; 1 direct; 2 auto: direct when the graph has 1 .. 128 end nodes,
 * else conjugate gradients).  H = M + U S U^T: M the band, U the components of the m distinct END nodes of the closures that lie off the band between two free
 * nodes, q = 6 m.  Per Gauss-Newton iteration, behind the same factorisation of the band: Z = M^-1 U (q band solves, one thread each, in one launch),
 * Wm = U^T Z = L L^T, Ks = I + L^T S L = Lk Lk^T, then x = apply(-g) and one step of iterative refinement x += apply(-g - H x), with
 * apply(b) = y - Z L^-T Ks^-1 L^T S U^T y, y = M^-1 b.  A fixed number of launches whatever the closures are.  A pivot of either Cholesky factorisation at or
 * below 1e-13 of its diagonal entry: _NOT_POSITIVE_DEFINITE (Ks is positive definite exactly when H is); not finite: _NON_FINITE; the outputs are then the inputs.
 * With m = 0 the solve is the single band solve.  max_pcg and pcg_tol are not used; pcg_iterations counts the single-right-hand-side band solves (two per
 * iteration, one with m = 0); result.solver is 1.  With option value 1 a graph of more than 128 end nodes is refused: ICET_ERR_UNSUPPORTED, nothing allocated,
 * the outputs untouched.
 * Test hook: icet_debug_pose_graph_step's arguments and conventions, the FIRST iteration with the direct solve whatever the option says.  HOST arrays the caller
 * sizes, or NULL: D, B n x 36 | A n_closures x 36 | g, x0 (before the refinement), x n x 6 | Z (6 n) x q, row-major | Wm, L, Ks, Lk q x q row-major (L, Lk: zeros
 * above the diagonal) | Pt n x 12 | chi_trial E | q_out K x n x 6 | ends m int32 (the end nodes, ascending).  ends_capacity (in): the m the caller sized the
 * arrays for; it must equal the graph's (else ICET_ERR_BAD_ARG; more than 128: ICET_ERR_UNSUPPORTED).  factor_status, wm_status, ks_status: the three
 * factorisations' statuses; band_solves as pcg_iterations; trial as in icet_pose_graph_step. */
typedef struct icet_pose_graph_direct_step {
    double *D, *B, *A, *g, *Z, *Wm, *L, *Ks, *Lk, *x0, *x, *Pt, *chi_trial, *q;
    int32_t* ends;
    int32_t ends_capacity;        /* in */
    int32_t m, factor_status, wm_status, ks_status, band_solves, trial;
    int32_t reserved;             /* zero */
    double  chi2_start, chi2_trial, max_dx;
} icet_pose_graph_direct_step;    /* 176 bytes */
icet_status icet_debug_pose_graph_direct(icet_ctx* ctx, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                         const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                         const icet_pose_graph_options* opt, int32_t K, const double* p, icet_pose_graph_direct_step* out);
/* MARGINAL COVARIANCES: how well each pose of a graph is known.  The graph arguments of icet_pose_graph_optimize (n through fixed) and its argument checks;
 * `poses` are the poses to evaluate at -- what the optimiser returned.  cov_out: n x 36 doubles, block (k, k) of H^-1 per node, H = sum J^T Omega J linearised
 * at `poses` with no damping, in the optimiser's tangent: delta = (translation, rotation vector) of the right update T Exp(delta), so rows and columns 0 .. 2
 * are metres in the node's OWN frame and 3 .. 5 radians.  Every block is symmetric bit for bit; a fixed node's block is zero.  The measurements (odo_X, clo_X)
 * are taken for symmetry of the call and do not enter the result.  H^-1 = M^-1 - P P^T + Q Q^T with the direct solve's Z, L, Lk (P = Z L^-T, Q = P Lk^-T) and
 * the diagonal blocks of M^-1 by the backward recurrence over the band's factor: a fixed number of launches.  The graph may have at most 128 end nodes (above:
 * ICET_ERR_UNSUPPORTED whatever option "pg_solver" says, nothing allocated, the outputs untouched).
 * result->status: 0, or ICET_POSE_GRAPH_NOT_POSITIVE_DEFINITE (a pivot of the band, of Wm or of Ks at or below 1e-13 of its diagonal entry) or _NON_FINITE (a
 * pivot that is not finite: a pose or an information that is not); factor_status, wm_status, ks_status say which.  Every free node's block is then quiet NaN
 * and every fixed node's zero.  The status is a RESULT: the call returns ICET_OK.
 * The first form takes HOST arrays; in the _device form poses, odo_X, odo_info, clo_X, clo_info and cov_out are DEVICE pointers (cov_out 8-byte aligned); ci, cj,
 * fixed and result stay on the host.  Both synchronise.  The context's parked keyframe and workspace are not touched.  ICET_ERR_BAD_ARG: as
 * icet_pose_graph_optimize, with cov_out and result in the place of poses_out and result. */
typedef struct icet_pose_graph_marginals_result {
    int32_t status;               /* 0, ICET_POSE_GRAPH_NOT_POSITIVE_DEFINITE or ICET_POSE_GRAPH_NON_FINITE */
    int32_t m;                    /* end nodes */
    int32_t factor_status, wm_status, ks_status;
    int32_t reserved;             /* zero */
} icet_pose_graph_marginals_result;   /* 24 bytes */
icet_status icet_pose_graph_marginals(icet_ctx* ctx, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                      const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                      double* cov_out, icet_pose_graph_marginals_result* result);
icet_status icet_pose_graph_marginals_device(icet_ctx* ctx, int32_t n, const float* d_poses, const float* d_odo_X, const float* d_odo_info, int32_t n_closures,
                                             const int32_t* ci, const int32_t* cj, const float* d_clo_X, const float* d_clo_info, const uint8_t* fixed,
                                             double* d_cov_out, icet_pose_graph_marginals_result* result);
/* Test hook: icet_pose_graph_marginals on HOST arrays with its intermediate arrays copied out.  HOST arrays the caller sizes, or NULL: D, B n x 36 | A
 * n_closures x 36 | band_cov n x 36 (the diagonal blocks of M^-1, the identity at a fixed node; left alone where the band did not factor) | cov n x 36 | ends m
 * int32.  ends_capacity (in) as in icet_pose_graph_direct_step; reserved zero. */
typedef struct icet_pose_graph_marginals_debug {
    double *D, *B, *A, *band_cov, *cov;
    int32_t* ends;
    int32_t ends_capacity;        /* in */
    int32_t reserved;             /* zero */
    icet_pose_graph_marginals_result result;
} icet_pose_graph_marginals_debug;    /* 80 bytes */
icet_status icet_debug_pose_graph_marginals(icet_ctx* ctx, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                            const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                            icet_pose_graph_marginals_debug* out);
/* COVARIANCE COLUMNS: how well two poses are known relative to each other.  The graph arguments, H, the tangent and the argument checks of
 * icet_pose_graph_marginals; `targets` (HOST) names 1 .. 32 distinct nodes.  cols_out: n_targets x n x 36 doubles, cols_out[t][k] is block (k, targets[t]) of
 * H^-1, row-major 6 x 6: rows are node k's tangent, columns the target's.  No damping; the measurements do not enter.  cov_out (n x 36, may be NULL) carries
 * the bits of icet_pose_graph_marginals on the same inputs, and so does cols_out[t][targets[t]]: it is copied from that result.  A block whose row node or
 * target is fixed (node 0 included) is +0.0 in every entry.  block (k, t) = [M^-1](k, t) - P_k P_t^T + Q_k Q_t^T with the marginals' P and Q: the marginals'
 * launches, one band solve for the targets' 6 x n_targets unit columns, one launch for the targets' P_t and Q_t and one with a workgroup per node.
 * result: as icet_pose_graph_marginals.  After a failed factorisation (status 2 or 3) every block between two free nodes is quiet NaN and every block that
 * touches a fixed node zero; the call returns ICET_OK.  Refused with nothing allocated and the outputs untouched: more than 128 end nodes
 * (ICET_ERR_UNSUPPORTED, whatever "pg_solver" says); n_targets outside 1 .. 32, a target out of range, a duplicate target, or a NULL targets, cols_out or
 * result (ICET_ERR_BAD_ARG).  In the _device form cols_out and cov_out are DEVICE pointers too (8-byte aligned).  Both forms synchronise and give the same bits,
 * run to run and form to form.  The context's parked keyframe and workspace are not touched. */
#define ICET_PG_MAX_TARGETS 32
icet_status icet_pose_graph_covariance_columns(icet_ctx* ctx, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures,
                                               const int32_t* ci, const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed,
                                               int32_t n_targets, const int32_t* targets, double* cols_out, double* cov_out,
                                               icet_pose_graph_marginals_result* result);
icet_status icet_pose_graph_covariance_columns_device(icet_ctx* ctx, int32_t n, const float* d_poses, const float* d_odo_X, const float* d_odo_info,
                                                      int32_t n_closures, const int32_t* ci, const int32_t* cj, const float* d_clo_X, const float* d_clo_info,
                                                      const uint8_t* fixed, int32_t n_targets, const int32_t* targets, double* d_cols_out, double* d_cov_out,
                                                      icet_pose_graph_marginals_result* result);
/* THE COVARIANCE GATE: is a candidate closure plausible under what the graph knows?  Candidate c (gi[c], gj[c] on the HOST; 1 <= n_cand <= 512) is a closure
 * that is NOT in the graph yet: keyframe node gi[c] seen from live node gj[c], with the measurement cand_X[c] (as clo_X) and its 6 x 6 covariance cand_cov[c]
 * (the record's own, used as 0.5 (c + c^T) in double).  Per candidate, in double: e is the optimiser's residual of edge (gi, gj) with that measurement at
 * `poses`, J_i, J_j its central-difference Jacobians, and
 *     S = J_i Sigma_ii J_i^T + J_i Sigma_ij J_j^T + J_j Sigma_ji J_i^T + J_j Sigma_jj J_j^T + cov,      d2 = e^T S^-1 e
 * with Sigma_ii, Sigma_jj the marginals and Sigma_ij the covariance column of target gj: ONE columns run whose targets are the distinct nodes among gj,
 * ascending (more than 32 of them: ICET_ERR_BAD_ARG), then one workgroup per candidate.  d2 goes through a 6 x 6 Cholesky factorisation of S: a pivot at or
 * below 1e-13 of its diagonal entry gives cand_status[c] 2, one that is not finite 3, otherwise 0.  d2_out[c] is d2, or quiet NaN behind status 2 or 3 or
 * behind a failed factorisation of the graph (result->marg.status); res_cov_out[c] (may be NULL) is S, symmetric bit for bit.  result->rejected counts the
 * candidates whose d2 is not below `threshold`; a threshold <= 0 means ICET_PG_ROBUST_DEFAULT_SCALE.  gi[c] == gj[c], an index out of range or n_cand
 * outside 1 .. 512: ICET_ERR_BAD_ARG; the refusals of icet_pose_graph_covariance_columns hold, nothing allocated, the outputs untouched.
 * CAVEAT: a candidate must not already be an edge of the graph -- its noise would be counted twice, in Sigma and in cov.
 * The first form takes HOST arrays; in the _device form cand_X, cand_cov, d2_out, res_cov_out and cand_status are DEVICE pointers too.  Both synchronise. */
typedef struct icet_pose_graph_gate_result {
    icet_pose_graph_marginals_result marg;
    int32_t n_targets;            /* the distinct nodes among gj */
    int32_t rejected;             /* candidates whose d2 is not below the threshold */
} icet_pose_graph_gate_result;    /* 32 bytes */
icet_status icet_pose_graph_gate(icet_ctx* ctx, int32_t n, const float* poses, const float* odo_X, const float* odo_info, int32_t n_closures, const int32_t* ci,
                                 const int32_t* cj, const float* clo_X, const float* clo_info, const uint8_t* fixed, int32_t n_cand, const int32_t* gi,
                                 const int32_t* gj, const float* cand_X, const float* cand_cov, double threshold, double* d2_out, double* res_cov_out,
                                 int32_t* cand_status, icet_pose_graph_gate_result* result);
icet_status icet_pose_graph_gate_device(icet_ctx* ctx, int32_t n, const float* d_poses, const float* d_odo_X, const float* d_odo_info, int32_t n_closures,
                                        const int32_t* ci, const int32_t* cj, const float* d_clo_X, const float* d_clo_info, const uint8_t* fixed, int32_t n_cand,
                                        const int32_t* gi, const int32_t* gj, const float* d_cand_X, const float* d_cand_cov, double threshold, double* d_d2_out,
                                        double* d_res_cov_out, int32_t* d_cand_status, icet_pose_graph_gate_result* result);
/* The optimiser's solver alone, as a test hook.  The odometry chain of a pose graph makes its normal equations block tridiagonal (6 x 6 blocks).
 * ONE symmetric positive definite block-tridiagonal system through the block Cholesky factorisation and the two sweeps, in double, one workgroup.
 * HOST arrays of doubles: diag n x 36, sub n x 36 (sub[k]: the block at (k, k - 1); sub[0] zero), rhs and x n x 6; *status 0, or ICET_BAND_NOT_POSITIVE_DEFINITE
 * (a pivot at or below 1e-13 of its diagonal entry) / ICET_BAND_NON_FINITE (a NaN or infinite pivot): x is then rhs.  1 <= n <= 4096.  Synchronises. */
#define ICET_BAND_NOT_POSITIVE_DEFINITE 2
#define ICET_BAND_NON_FINITE 3
icet_status icet_debug_block_tridiag(icet_ctx* ctx, int32_t n, const double* diag, const double* sub, const double* rhs, double* x, int32_t* status);

/* --- the voxel map: many scans, each at a pose, fused into one centroid and one count per occupied cell, in HBM ---------------------
 * A map borrows a context like a keyframe store (destroy it before the context) and owns its memory: an open-addressing hash table of 2^table_log2 entries
 * of 40 bytes (key, count, three offset sums, all 64-bit integers; 72 bytes more once icet_voxel_map_enable_shape has run: "the voxel map's shape" below).  THE RULE, for a row (x, y, z) of a scan at the pose T = [R | t] (4 x 4 row-major
 * float32, p_world = R p + t), every operation IEEE double, rounded once, nothing contracted:
 *   1. a row with a non-finite coordinate is counted in points_nonfinite and skipped;
 *   2. d2 = (x x + y y) + z z; the row is kept iff d2 > min_range^2 and (max_range <= 0 or d2 <= max_range^2) -- at min_range = 0 exactly the all-zero rows go;
 *   3. w_a = ((R[a][0] x + R[a][1] y) + R[a][2] z) + t[a], s_a = w_a (1 / (double)cell), c_a = floor(s_a); unless |c_a| < 2^20 on all three axes the row is
 *      counted in points_outside and skipped (a NaN or infinity in the pose ends here);
 *   4. u_a = s_a - c_a, q_a = min(floor(u_a 2^32), 2^32 - 1);
 *   5. key = (c_x + 2^20) << 42 | (c_y + 2^20) << 21 | (c_z + 2^20); the cell of the key gets count += sign and sum_a += sign q_a, in 64-bit integers.
 * The centroid of a cell of count n >= 1 is (float)(((double)c_a + (double)sum_a / ((double)n 2^32)) (double)cell).  Every sum is an integer, so a map holds
 * the same bits whatever the order, the call boundaries or the launch shape, and REMOVING a scan (sign -1) at the pose it was added at undoes it exactly:
 * remove at the old poses + add at the corrected ones is bit for bit a fresh build.
 * CREATE: cell finite and > 0, min_range and max_range finite, table_log2 10 .. 30, flags and the reserved words 0, else ICET_ERR_BAD_ARG; a failed allocation
 *   ICET_ERR_NOMEM (*out stays NULL).  The map starts empty.
 * ADD: n scans (HOST descriptors of DEVICE rows, N x 3 column-major float32, ld >= n, padding never read, n = 0 allowed) at n poses -- HOST n x 16 floats
 *   (add_device) or DEVICE n x 16 floats, 4-byte aligned (add_posed_device: what icet_pose_graph_optimize_device leaves in d_poses_out) --, sign +1 (add) or
 *   -1 (remove); one launch for the whole call, asynchronous on the context's stream.  A row that finds no free entry is counted in points_dropped and raises
 *   ICET_VOXEL_MAP_TABLE_FULL: it is never lost silently (a full table is not rehashed).  Option "map_lds" (icet_set_option; default 1): a block first
 *   reduces its rows in an LDS table and flushes each distinct cell once; 0: one global update per row.  Same contents either way.
 * STATS: the running totals since the last clear, and the cells as they are now, counted for min_points (cells_out: count >= max(1, min_points)).  Synchronises.
 * EXTRACT: the cells with count >= max(1, min_points), sorted by key ascending (x-major, reproducible), as a scan: d_xyz N x 3 column-major float32 with
 *   leading dimension ld >= cap_rows; d_count and d_key (either may be NULL) the cells' counts and keys.  With cap_rows < cells_out the cap_rows lowest keys
 *   are written and ICET_VOXEL_MAP_TRUNCATED is set.  extract_device writes DEVICE pointers, extract HOST pointers; both synchronise and fill *out (may be NULL).
 * CLEAR empties the table and zeroes the totals (asynchronous).
 * Refusals (ICET_ERR_BAD_ARG, the reason in icet_voxel_map_last_error, nothing touched): a NULL map or array, n < 0, a bad descriptor, sign not +1 / -1,
 *   cap_rows < 0, ld < cap_rows.  There is no CPU fallback.  The context's parked keyframe, workspace and every store are not touched. */
typedef struct icet_voxel_map icet_voxel_map;
typedef struct icet_voxel_map_params {
    float cell;                   /* edge of a cell, metres */
    float min_range, max_range;   /* rows with d2 <= min_range^2 or (max_range > 0) d2 > max_range^2 are skipped */
    int32_t table_log2;           /* 10 .. 30 */
    int32_t flags;                /* 0 */
    int32_t reserved[3];
} icet_voxel_map_params;          /* 32 bytes */
#define ICET_VOXEL_MAP_OK 0
#define ICET_VOXEL_MAP_TABLE_FULL 1       /* status bits */
#define ICET_VOXEL_MAP_NEGATIVE 2         /* a cell's count is below zero: a remove without its add */
#define ICET_VOXEL_MAP_TRUNCATED 4        /* (extract) fewer rows than cells_out were written */
/* (a struct tag without a typedef: the call below has the same name) */
struct icet_voxel_map_stats {
    int64_t points_in;            /* rows read, adds and removes */
    int64_t points_kept;          /* rows that reached a cell: adds minus removes */
    int64_t points_nonfinite, points_outside, points_dropped;
    int32_t cells_occupied;       /* count > 0 */
    int32_t cells_out;            /* count >= max(1, min_points) */
    int32_t cells_negative;       /* count < 0 */
    int32_t status;               /* ICET_VOXEL_MAP_* bits */
    int32_t reserved[2];
};                                /* 64 bytes */
icet_status icet_voxel_map_create(icet_ctx* ctx, const icet_voxel_map_params* p, icet_voxel_map** out);
icet_status icet_voxel_map_destroy(icet_voxel_map* map);
const char* icet_voxel_map_last_error(const icet_voxel_map* map);
icet_status icet_voxel_map_clear(icet_voxel_map* map);
icet_status icet_voxel_map_add_device(icet_voxel_map* map, int32_t n, const icet_dev_scan* scans, const float* poses, int32_t sign);
icet_status icet_voxel_map_add_posed_device(icet_voxel_map* map, int32_t n, const icet_dev_scan* scans, const float* d_poses, int32_t sign);
icet_status icet_voxel_map_stats(icet_voxel_map* map, int32_t min_points, struct icet_voxel_map_stats* out);
icet_status icet_voxel_map_extract_device(icet_voxel_map* map, int32_t min_points, float* d_xyz, int64_t ld, int64_t cap_rows, int64_t* d_count, uint64_t* d_key,
                                          struct icet_voxel_map_stats* out);
icet_status icet_voxel_map_extract(icet_voxel_map* map, int32_t min_points, float* xyz, int64_t ld, int64_t cap_rows, int64_t* count, uint64_t* key,
                                   struct icet_voxel_map_stats* out);

/* --- the voxel map's query: sub-maps around poses, each in its pose's own frame, in one call -------------------------------------------
 * For each of n_q poses T = [R | t] (the map's POSE convention) the cells of the map within a range of t, laid out as a scan, so that a sub-map goes into
 * icet_keyframe_store_put_device / icet_keyframe_device_n with its row count read on the device.  THE RULE, for a cell of count n and centroid
 * m = (m_0, m_1, m_2) -- the three float32 values extract writes --, every operation IEEE double, rounded once, nothing contracted:
 *   1. if any of the 12 entries T[0 .. 11] is not finite the query yields 0 rows and status bit ICET_VOXEL_MAP_QUERY_BAD_POSE (host and device poses alike:
 *      a pose is never refused on the host);
 *   2. the cell takes part iff n >= max(1, min_points);
 *   3. d_a = (double)m_a - (double)t_a, d2 = (d_0 d_0 + d_1 d_1) + d_2 d_2; the cell is kept iff d2 > min_range^2 and (max_range <= 0 or d2 <= max_range^2),
 *      the squares taken in double from the float32 parameters -- the map's own range rule: a centroid exactly at t is dropped at min_range = 0;
 *   4. the row is (float)((R[0][a] d_0 + R[1][a] d_1) + R[2][a] d_2) for a = 0, 1, 2: R^T d, the inverse of the pose taken as the transpose (R is the
 *      caller's and is not checked); with flag ICET_VOXEL_MAP_QUERY_WORLD the row is m itself, bit for bit the row extract writes;
 *   5. a query's rows are in ascending key order, extract's; count (int64) and key (uint64) per row are optional outputs;
 *   6. total = the kept cells, rows = min(total, cap_rows); with total > cap_rows the cap_rows lowest keys are written and ICET_VOXEL_MAP_TRUNCATED is set for
 *      that query.  cap_rows = 0 with a NULL xyz is a count-only query: how a caller sizes its buffers.  Padding beyond rows is never written.
 * INDEX: the queries read a sorted index of the map -- the cells with count >= 1 by ascending key, as contiguous arrays of key, count and centroid, in buffers
 *   of its own (extract's results do not change).  add, remove and clear make it stale; icet_voxel_map_index rebuilds a stale index with extract's
 *   sequence (count, select, sort, centroids), which synchronises, fills *out (may be NULL) with the stats at min_points 1, and does nothing but that when the
 *   index is current.
 * QUERY: poses are HOST n_q x 16 floats (query_device) or DEVICE n_q x 16 floats, 4-byte aligned (query_posed_device: what icet_pose_graph_optimize_device
 *   leaves in d_poses_out); outs HOST descriptors of DEVICE memory; d_rows (required), d_total and d_status (either may be NULL) DEVICE int32 arrays of n_q
 *   entries.  Both calls rebuild a stale index first (and synchronise then, or when their own buffers grow); otherwise they are asynchronous on the context's
 *   stream and write nothing on the host.  1 <= n_q <= ICET_VOXEL_MAP_MAX_QUERIES.  Three launches: the cells are read in chunks of
 *   ICET_VOXEL_MAP_QUERY_CHUNK consecutive index entries and counted per (query, chunk); one block per query scans its counts and writes the three words; the
 *   test is repeated and the rows are written at chunk offset + wave prefix + lane prefix.  No atomics on global memory.  Option "map_query_prune"
 *   (icet_set_option; default 1): keys sort x-major, so a chunk whose x cells lie outside [floor((t_0 - max_range) / cell) - 1, floor((t_0 + max_range) / cell) + 1]
 *   is not tested for that query; 0 tests everything.  Same bits either way.
 * Refusals (ICET_ERR_BAD_ARG, the reason in icet_voxel_map_last_error, nothing touched): a NULL map or array, n_q out of range, cap_rows < 0, ld < cap_rows,
 *   cap_rows > 0 with a NULL xyz, a device pointer not aligned to its element, a non-finite min_range or max_range, unknown flag bits, nonzero reserved words. */
#define ICET_VOXEL_MAP_QUERY_BAD_POSE 8   /* status bit of a query: a non-finite entry in its pose */
#define ICET_VOXEL_MAP_QUERY_WORLD 1      /* flag: rows in the world frame */
#define ICET_VOXEL_MAP_MAX_QUERIES 256
#define ICET_VOXEL_MAP_QUERY_CHUNK 2048   /* index entries per block of a query */
typedef struct icet_voxel_map_query {
    float min_range, max_range;   /* cells with d2 <= min_range^2 or (max_range > 0) d2 > max_range^2 are dropped */
    int32_t min_points;           /* cells with count >= max(1, min_points) take part */
    int32_t flags;                /* ICET_VOXEL_MAP_QUERY_* */
    int32_t reserved[4];
} icet_voxel_map_query;           /* 32 bytes */
typedef struct icet_voxel_map_submap {
    float* xyz;                   /* DEVICE rows, N x 3 column-major float32; may be NULL with cap_rows 0 */
    int64_t ld, cap_rows;         /* ld >= cap_rows >= 0 */
    int64_t* count;               /* DEVICE, cap_rows entries, or NULL */
    uint64_t* key;                /* DEVICE, cap_rows entries, or NULL */
} icet_voxel_map_submap;          /* 40 bytes: a HOST descriptor of DEVICE memory */
icet_status icet_voxel_map_index(icet_voxel_map* map, struct icet_voxel_map_stats* out);
icet_status icet_voxel_map_query_device(icet_voxel_map* map, int32_t n_q, const float* poses, const icet_voxel_map_query* q, const icet_voxel_map_submap* outs,
                                        int32_t* d_rows, int32_t* d_total, int32_t* d_status);
icet_status icet_voxel_map_query_posed_device(icet_voxel_map* map, int32_t n_q, const float* d_poses, const icet_voxel_map_query* q, const icet_voxel_map_submap* outs,
                                              int32_t* d_rows, int32_t* d_total, int32_t* d_status);

/* --- the voxel map's visibility evidence: which cells later scans saw THROUGH, so that movers leave the map ----------------------------
 * A cell that any scan ever hit stays in the map; a car that drove past stays as ghost cells.  A cell is suspect when scans measured something further away
 * through it.  The evidence is a pure function of the map's index, the scans and the poses given: integers and minima only, independent of order, call
 * boundaries and launch shape.  THE RULE (icet_amd/csrc/icet_map_evidence.h), every operation IEEE double, rounded once, nothing contracted, division and
 * square root correctly rounded; W = 2^image_log2:
 *   A. the RANGE IMAGE of one scan, in the sensor's frame (no pose involved), for a row (x, y, z): a non-finite coordinate takes no part;
 *      d2 = (x x + y y) + z z, the row takes part iff d2 > min_range^2 (the map's max_range is not applied: a far return is evidence about everything in front
 *      of it); a = (|x| + |y|) + |z|, px = x / a, py = y / a; if z < 0: (px, py) <- ((1 - |py|) sgn(px), (1 - |px|) sgn(py)) with the old px, py on the right
 *      and sgn(v) = v < 0 ? -1 : +1 (the octahedral map); u = clamp(floor((px + 1) (W / 2)), 0, W - 1), v likewise from py, the double clamped before the
 *      conversion; the pixel v W + u keeps the MINIMUM of r = (float)sqrt(d2) over its rows, taken on the float's bits as uint32; all ones is an empty pixel;
 *   B. the NEAR IMAGE: near[v][u] = the minimum of the image over [v - window, v + window] x [u - window, u + window] clipped to the image (no wrap);
 *   C. one cell (centroid m, the three float32 values extract writes) against one scan at the pose T = [R | t]: a non-finite entry among T[0 .. 11] -- the scan
 *      gives no evidence and counts in scans_bad_pose; d_a = (double)m_a - (double)t_a, p_a = (R[0][a] d_0 + R[1][a] d_1) + R[2][a] d_2,
 *      d2 = (p_0 p_0 + p_1 p_1) + p_2 p_2; the scan takes part for the cell iff d2 > min_range^2 and d2 <= max_range^2; the pixel of p by A; an empty near
 *      pixel is no evidence; rc = sqrt(d2), rn = (double)near, mg = (double)margin: MISS iff rn > rc + mg, else AGREE iff rn >= rc - mg, else the cell is
 *      occluded, which is no evidence;
 *   D. per cell: miss and agree are int32 sums over the call's scans; transient = miss >= max(1, min_miss) && (int64)miss > (int64)agree_factor * agree.
 * The evidence covers the cells of the index (count >= 1) in index order: the order of extract at min_points 1 and of a world query of everything.
 * evidence_device (HOST poses) and evidence_posed_device (DEVICE poses, 4-byte aligned) rebuild a stale index first, zero the evidence, accumulate it over the
 *   n >= 0 scans (n = 0: all zero), take the decision, and with out != NULL fill *out and synchronise (out == NULL: asynchronous unless the index was stale or
 *   a buffer grew).  The scans are imaged in batches (option "map_evidence_batch": 0, the default, as many as fit 64 MiB of images, 1 .. 256; same bits for every
 *   value); a scan whose run of x cells misses a chunk of the index is not tested against it (option "map_evidence_prune", default 1; same bits).
 * The evidence belongs to the index it was computed on: add, remove and clear make it stale together with the index.  evidence_fetch_device copies what the map
 *   holds into DEVICE arrays of cap >= the index's cells (any of the three may be NULL; *rows_out, HOST, may be NULL), on the context's stream.
 * ICET_VOXEL_MAP_QUERY_STATIC in icet_voxel_map_query.flags: transient cells take no part in the query.  Without current evidence such a query is refused.
 * Refusals (ICET_ERR_BAD_ARG, the reason in icet_voxel_map_last_error, nothing touched): a NULL map or record, a NULL array with n > 0, n < 0, a bad descriptor,
 *   a non-finite parameter or one out of its range, unknown flags, a misaligned device pointer; a fetch without current evidence or with cap below the index.
 * No CPU fall-back.  Stores, the context's workspace and extract's buffers are not touched. */
#define ICET_VOXEL_MAP_QUERY_STATIC 2     /* flag of a query: the cells the current evidence calls transient take no part */
typedef struct icet_voxel_map_evidence {
    float min_range, max_range, margin;   /* finite; max_range > 0; margin >= 0 */
    int32_t image_log2;                   /* 4 .. 10 */
    int32_t window;                       /* 0 .. 2 */
    int32_t min_miss, agree_factor;       /* >= 0 */
    int32_t flags;                        /* 0 */
} icet_voxel_map_evidence;        /* 32 bytes */
struct icet_voxel_map_evidence_stats {
    int64_t rows_imaged;          /* rows that entered a range image (a scan with an unusable pose is imaged too) */
    int32_t cells, cells_transient, scans_used, scans_bad_pose;
    int32_t reserved[2];
};                                /* 32 bytes */
icet_status icet_voxel_map_evidence_device(icet_voxel_map* map, int32_t n, const icet_dev_scan* scans, const float* poses, const icet_voxel_map_evidence* e,
                                           struct icet_voxel_map_evidence_stats* out);
icet_status icet_voxel_map_evidence_posed_device(icet_voxel_map* map, int32_t n, const icet_dev_scan* scans, const float* d_poses, const icet_voxel_map_evidence* e,
                                                 struct icet_voxel_map_evidence_stats* out);
icet_status icet_voxel_map_evidence_fetch_device(icet_voxel_map* map, int32_t* d_miss, int32_t* d_agree, uint8_t* d_transient, int64_t cap, int64_t* rows_out);

/* --- the voxel map's shape: a covariance, its eigenvalues and a normal per cell, from integer second moments ---------------------------
 * A plain map knows where a surface is; a SHAPED map also knows how its points lie in each cell.  THE RULE (icet_amd/csrc/icet_map_shape.h), for a kept row with
 * the offsets q_a of step 4 of the map's rule: h_a = q_a >> 16 (0 .. 65535); beside count and sum the cell of the key gets nine more 64-bit two's-complement words,
 *   S_x S_y S_z M_xx M_xy M_xz M_yy M_yz M_zz:   S_a += sign h_a,   M_ab += sign h_a h_b.
 * h_a h_b < 2^32, so a cell still holds 2^32 rows; the resolution is cell / 65536.  The words are sums of integers: they depend on the multiset of (row, pose,
 * sign) only, and remove at the old pose + add at the corrected one is a rebuild, bit for bit, moments included.
 * COVARIANCE of a cell of count n >= 1, in the world frame, every operation IEEE double, rounded once, nothing contracted, u64 -> double to nearest even:
 *   m_a = (double)S_a / (double)n, E_ab = (double)M_ab / (double)n, k = (double)cell 2^-16, k2 = k k, C_ab = (E_ab - m_a m_b) k2; cov = (float)C in the order
 *   xx, xy, xz, yy, yz, zz.  No quantisation correction.  A cell of one row gives exactly zero.
 * EIGENVALUES AND NORMAL: a cyclic Jacobi on the double C with V = I at the start, 6 sweeps over the pairs (0,1), (0,2), (1,2); a pair with C_pq == 0 is
 *   skipped; theta = (C_qq - C_pp) / (2 C_pq), t = sgn(theta) / (|theta| + sqrt(theta theta + 1)) with sgn(0) = +1, c = 1 / sqrt(t t + 1), s = t c.  evals: the
 *   diagonal ascending, as computed (a tiny negative value stays negative), float32.  normal: the column of V of the smallest eigenvalue, ties to the lowest
 *   column, rounded to float32, then signed so that its component of largest magnitude is positive, the lowest axis winning a tie.  One row: zeros and (1, 0, 0).
 * ENABLE: icet_voxel_map_enable_shape allocates and zeroes the words (72 bytes per entry more) on a map that has read no row since it was created or last
 *   cleared -- else ICET_ERR_BAD_ARG --, and does nothing on a shaped map.  ICET_ERR_NOMEM when the allocation fails: the map stays plain.  From then on add and
 *   remove carry the words (both forms of option "map_lds"), clear zeroes them, and extract, stats, index, the queries and the evidence read the map as before.
 * EXTRACT_SHAPE: extract's rows -- the same cells, order, bits of xyz / count / key, and TRUNCATED rule -- and per row the columns of *shape, each column-major
 *   over shape->ld >= cap_rows; any of the four pointers may be NULL.  extract_shape_device takes DEVICE pointers, extract_shape HOST pointers; both synchronise.
 * Refusals (ICET_ERR_BAD_ARG, nothing touched): extract's, a map without shape, a NULL descriptor, shape->ld < cap_rows, nonzero flags or reserved, a misaligned
 *   device pointer.  No CPU fall-back. */
typedef struct icet_voxel_map_shape {
    float* cov;                   /* 6 columns: xx xy xz yy yz zz, square metres */
    float* normal;                /* 3 columns */
    float* evals;                 /* 3 columns, ascending */
    uint64_t* moments;            /* 9 columns: the raw words */
    int64_t ld;                   /* >= cap_rows */
    int32_t flags;                /* 0 */
    int32_t reserved;             /* 0 */
} icet_voxel_map_shape;           /* 48 bytes */
icet_status icet_voxel_map_enable_shape(icet_voxel_map* map);
icet_status icet_voxel_map_extract_shape_device(icet_voxel_map* map, int32_t min_points, float* d_xyz, int64_t ld, int64_t cap_rows, int64_t* d_count, uint64_t* d_key,
                                                const icet_voxel_map_shape* shape, struct icet_voxel_map_stats* out);
icet_status icet_voxel_map_extract_shape(icet_voxel_map* map, int32_t min_points, float* xyz, int64_t ld, int64_t cap_rows, int64_t* count, uint64_t* key,
                                         const icet_voxel_map_shape* shape, struct icet_voxel_map_stats* out);

/* --- registration against the map's Gaussians (a SHAPED map) -------------------------------------------------------------------------------
 * Scans at start poses in, refined poses out: NDT-style point-to-distribution Gauss-Newton against the cells of the map as they lie in the table, for many scans
 * or many start hypotheses of one scan in one call, nothing leaving the device.  THE RULE (icet_amd/csrc/icet_map_register.h is the authority on the order of
 * the operations; IEEE double, one rounding per operation, nothing contracted, no transcendental):
 *   a cell of count n >= max(1, min_points) has the mean mu_a = ((double)c_a + (double)sum_a / ((double)n 2^32)) (double)cell, the covariance C of "the voxel
 *   map's shape", C' = C + sigma_min^2 I and the weight W = C'^-1 (adjugate over determinant); a determinant that is not finite and > 0 leaves the cell out.
 *   A row p of a scan at the pose P = (R, t): non-finite rows and rows outside (min_range, max_range] of THIS call take no part; every other row is SCORED:
 *   r = R p, w = r + t; a row outside the grid, in no cell or in an unusable one is a MISS and costs exactly `scale`; else d = w - mu, a = W d, s = d . a,
 *   the row costs rho = scale s / (scale + s) (Geman-McClure) and weighs omega = (scale / (scale + s))^2.  cost = sum rho.
 *   TANGENT: delta = (rho_t, om), world-aligned at the sensor origin: w' = w + rho_t + om x r, J = [I | -[r]x]; g = sum omega J^T a, info = sum omega J^T W J
 *   (the upper triangle by rows, 21 doubles).  RETRACTION: R <- E(om) R, t <- t + rho_t, E the rotation of icet_pose_from_twist((0, om), 1), |om| <= 1.
 *   LOOP: Levenberg-Marquardt, (info + lambda diag(info)) delta = -g by a 6 x 6 Cholesky; a trial is accepted iff its cost is finite and below the current one
 *   (lambda / 10, not below 1e-9), else lambda x 10 (above 1e9: STALLED); CONVERGED when an accepted step has |rho_t| <= tol_t and |om| <= tol_r.
 *   NEIGHBOURHOODS (flags): 0 scores a row against its own cell, as above.  ICET_VOXEL_MAP_REG_NEIGHBOURS_7 looks at own, -x, +x, -y, +y, -z, +z in this order,
 *   ICET_VOXEL_MAP_REG_NEIGHBOURS_27 at own, then the other 26 offsets (dx, dy, dz), dx slowest, each over -1, 0, 1; a neighbour outside the grid is skipped and a
 *   row outside the grid stays a miss.  Every usable cell among them gives s = d . W d as above; the row is scored against the cell with the SMALLEST s (a cell
 *   wins iff its s is below the best so far, which starts at +infinity: a tie stays with the earlier cell, a NaN or infinite s never wins) and takes that cell's
 *   rho, omega, g and info terms; without a winner it is a miss.  A row still costs at most `scale`, row by row rho(27) <= rho(7) <= rho(own), and the cost is
 *   continuous where a row crosses a face between two usable cells.  Everything else -- the sums, the loop, the statuses, the Gaussians and when they are stale --
 *   is the same; flags = 0 runs the same code and gives the same bits as before the neighbourhoods existed.
 * max_iters = 0 scores the given poses.  Asynchronous on the context's stream: a fixed number of launches (the Gaussians if they are stale, then 1 + max_iters
 * passes of two kernels), no host round trip.  The Gaussians are rebuilt after add, remove, clear and enable_shape and when sigma_min or min_points change.
 * Queries may share a scan descriptor (several start poses of one scan).  Sums in a fixed order: the same call gives the same bits, and a query's bits depend on
 * neither its place in the call nor its neighbours.
 * Refusals (ICET_ERR_BAD_ARG, the reason in icet_voxel_map_last_error, nothing touched): a map without shape, a NULL map or array, n_q outside 1 ..
 *   ICET_VOXEL_MAP_MAX_QUERIES, a bad descriptor, sigma_min, scale or lambda0 not finite and > 0, max_iters outside 0 .. 64, negative tolerances, non-finite
 *   ranges, flags other than 0 or ONE of ICET_VOXEL_MAP_REG_NEIGHBOURS_7 / _27 (both bits, or any other bit), nonzero reserved words, d_records or d_poses
 *   misaligned.  No CPU fall-back. */
#define ICET_VOXEL_MAP_REG_CONVERGED 0
#define ICET_VOXEL_MAP_REG_ITERATION_CAP 1         /* still running after pass max_iters (every scored pose of max_iters = 0) */
#define ICET_VOXEL_MAP_REG_STALLED 2
#define ICET_VOXEL_MAP_REG_NO_OVERLAP 3            /* fewer than min_matched rows matched at the start pose: pose = the start pose's bits */
#define ICET_VOXEL_MAP_REG_BAD_POSE 4              /* a non-finite entry in the start pose */
#define ICET_VOXEL_MAP_REG_MAX_ITERS 64
#define ICET_VOXEL_MAP_REG_NEIGHBOURS_7 2          /* icet_voxel_map_register_params.flags: a row is scored against the best of its own cell and the six across its faces */
#define ICET_VOXEL_MAP_REG_NEIGHBOURS_27 4         /* the best of the 27 cells around it */
typedef struct icet_voxel_map_register_params {
    float min_range, max_range;   /* of this call, as icet_voxel_map_params' (max_range <= 0: no limit) */
    double sigma_min;             /* the live point's own noise, metres (0.02) */
    double scale;                 /* the robust scale in chi2 units, and the cost of a miss (11.3449: the 99 % quantile of chi2 with three degrees of freedom) */
    double tol_t, tol_r;          /* metres (1e-4), radians (1e-5) */
    double lambda0;               /* 1e-3 */
    int32_t min_points;           /* 5 */
    int32_t min_matched;          /* 50 */
    int32_t max_iters;            /* 20; 0 .. 64 */
    int32_t flags;                /* 0: a row is scored against its own cell; or ONE of ICET_VOXEL_MAP_REG_NEIGHBOURS_* */
    int32_t reserved[2];          /* 0 */
} icet_voxel_map_register_params; /* 72 bytes; NULL: the defaults */
typedef struct icet_voxel_map_registration {
    float pose[16];               /* the pose returned, 4 x 4 row-major */
    double info[21];              /* sum omega J^T W J at that pose, upper triangle by rows, in the tangent (rho_t, om) above */
    double g[6];                  /* sum omega J^T a at that pose */
    double cost, cost_start;      /* sum rho at the pose returned and at the start pose */
    double lambda;
    int32_t rows_scored, rows_matched;
    int32_t iterations, accepted; /* passes after the first, and the trials among them that were accepted */
    int32_t status;               /* ICET_VOXEL_MAP_REG_* */
    int32_t reserved;
} icet_voxel_map_registration;    /* 328 bytes, 8-byte aligned */
/* one row of icet_debug_voxel_map_register_terms */
typedef struct icet_voxel_map_register_term {
    uint64_t key;                 /* the row's cell (all ones: outside the grid or not scored) */
    int32_t cls;                  /* the map rule's class: 0 scored, 1 non-finite, 2 range, 3 outside the grid */
    int32_t matched;              /* 0: a miss; else 1 + the place of the cell the row is scored against in the order of its neighbourhood (1: its own cell) */
    double s, omega, rho;         /* zero for a row that is not scored; a miss: s 0, omega 0, rho scale; under a neighbourhood: the winning cell's */
    double g[6], H[21];
} icet_voxel_map_register_term;   /* 256 bytes */
icet_status icet_voxel_map_register_device(icet_voxel_map* map, int32_t n_q, const icet_dev_scan* scans, const float* poses,
                                           const icet_voxel_map_register_params* params, icet_voxel_map_registration* d_records);
icet_status icet_voxel_map_register_posed_device(icet_voxel_map* map, int32_t n_q, const icet_dev_scan* scans, const float* d_poses,
                                                 const icet_voxel_map_register_params* params, icet_voxel_map_registration* d_records);
/* For ONE query (a scan and a HOST pose): the row pass of the start pose, and per row of the scan one record into d_terms (DEVICE, scan->n records). */
icet_status icet_debug_voxel_map_register_terms(icet_voxel_map* map, const icet_dev_scan* scan, const float* pose, const icet_voxel_map_register_params* params,
                                                icet_voxel_map_register_term* d_terms);

/* --- the voxel map kept: save, load, merge (the file format and its validation: icet_amd/csrc/icet_map_snapshot.h) --------------------------
 * Every per-cell word of a map is a 64-bit integer sum, so maps in ONE frame are additive cell by cell: adding the words of map B's cells to map A's gives, bit
 * for bit, the map built from the scans of both, and subtracting them gives A back.  Save, load, merge and growing a table are that one operation -- the words
 * of a set of cells into a table with sign +1 or -1 -- with the source in a file or in another table.
 * THE FILE (little-endian, every part on a 16-byte boundary, reserved bytes and padding zero, every byte under a checksum): a 128-byte header -- magic
 *   "ICETVXM1", version, the bit patterns of cell / min_range / max_range, the shaped flag, words per entry W (5: key, count, three sums; a shaped map 14: and
 *   the nine moment words), the entry count n, the five running totals, the file's size, the payload's and the header's checksum -- and W columns of n u64
 *   words.  Written: every claimed entry with a non-zero value word, by ascending key; a cell emptied by a remove is not written, a negative count or a zero
 *   count beside non-zero sums is.  The file is a function of the map's contents alone: not of the table's size, the order of the adds, option "map_lds", the
 *   call boundaries or the chunk size.
 * SAVE runs behind what was enqueued, synchronises, and writes `path`.tmp, renamed when complete: a failed save leaves nothing at `path`.  The map is not changed
 *   (its index, evidence and Gaussians stay current).  The payload moves in chunks of option "map_snapshot_chunk_entries" entries (icet_set_option on the
 *   map's context; default and 0: 2^20; same bytes for every value).
 * LOAD reads and validates the whole file on the host, holds it against the map, counts on the device how many of its keys the table does not hold yet, and
 *   only then adds the words times `sign`.  The file's cell must equal the map's bit for bit; a shaped file into a plain map leaves the moment columns out; a
 *   plain file into a shaped map is refused (the moments would no longer belong to the counts); the ranges are recorded and reported, not compared.  When
 *   claimed entries + new keys exceed the table's size the load is refused with nothing touched (below that bound no insert can fail: a loaded cell is never
 *   dropped).  The file's five totals are added to the map's, or with sign -1 ALL FIVE are subtracted, points_in included -- unlike a remove, which keeps
 *   counting the rows it reads: a load or merge at -1 undoes the same load or merge at +1 exactly, totals too.  Afterwards the map is as after an add: index,
 *   evidence and Gaussians are stale, and icet_voxel_map_enable_shape is refused until the next clear.  Synchronises.
 * MERGE is load with the source in device memory: dst and src on the same context, dst != src, the same cell, shape and capacity rules, the same effects on
 *   dst; src is only read.  Growing a full table (ICET_VOXEL_MAP_TABLE_FULL) is a merge into a new, larger map.  Asynchronous behind its capacity check.
 * Refusals (ICET_ERR_BAD_ARG, the reason in icet_voxel_map_last_error, nothing touched): a NULL argument, a path that cannot be opened, a file the validation
 *   refuses, a cell mismatch, the shape rule, the capacity bound, sign not +1 / -1, two contexts in a merge.  A save whose file cannot be written to the
 *   end -- a full disk, a failed seek, write, close or rename -- answers ICET_ERR_BAD_ARG as well (the status set has nothing nearer): the message names
 *   the failed step and the system's reason, which is how a caller tells it from a bad path; the temporary file is removed.  No CPU fall-back.
 * The sorted cells of a save and the staging of a save or a load (one device and two pinned buffers of min(chunk, entries) x W words) stay with the map and
 *   grow on demand; icet_voxel_map_destroy frees them. */
/* (a struct tag without a typedef: the call below has the same name) */
struct icet_voxel_map_snapshot_info {
    float cell, min_range, max_range;         /* of the map that was saved */
    int32_t shaped;                           /* 1: the file carries the nine moment words */
    int32_t words_per_entry;                  /* 5 or 14 */
    int32_t reserved0;
    int64_t entries;
    int64_t points_in, points_kept, points_nonfinite, points_outside, points_dropped;
    int64_t file_bytes;
    uint64_t payload_checksum;
    int32_t reserved[2];
};                                /* 96 bytes */
icet_status icet_voxel_map_save(icet_voxel_map* map, const char* path);
icet_status icet_voxel_map_load(icet_voxel_map* map, const char* path, int32_t sign);
icet_status icet_voxel_map_snapshot_info(const char* path, struct icet_voxel_map_snapshot_info* out);
icet_status icet_voxel_map_merge_device(icet_voxel_map* dst, icet_voxel_map* src, int32_t sign);

/* --- deskew: undo a sweep's motion in many scans, in one call ---------------------------------------------------------------------------
 * A spinning lidar takes 50 - 100 ms per sweep; the rows of one scan are taken from a moving sensor.  A deskewer carries every row into the sensor frame at ONE
 * instant of the sweep, given the sweep's motion as a twist and a time (or a column index) per row.  It borrows a context like a store or a map (destroy it
 * before the context), owns its memory and borrows only the stream.
 * MOTION: a twist xi = (rho, phi), six doubles; T(s) = exp(s xi) = [exp(s phi^) | V(s phi) s rho] is the sensor's pose at sweep fraction s in the sensor frame
 * at s = 0 (the store's POSE convention: p_0 = R p_s + t).  Under constant velocity over a frame period xi = log(icet_pose_step_from_x(X)).  A row taken at s
 * is carried into the frame at s_ref (0: sweep start, 1: sweep end) by p' = exp((s - s_ref) xi) p.
 * THE RULE (icet_amd/csrc/icet_deskew.h), per row i with float32 coordinates x, y, z; every operation IEEE double, rounded once, nothing contracted:
 *   1. a non-finite coordinate: the row's bits are copied, class nonfinite;
 *   2. x, y and z all 0 (either sign): the bits are copied (the invalid returns of a real scan stay exact zeros), class zero;
 *   3. the row's time tau: ICET_DESKEW_TIME_ARRAY (double)time[i], a non-finite one copies the bits, class bad_time; ICET_DESKEW_TIME_COLUMN_FAST
 *      (i mod period) + 0.5, period the columns of an organised scan whose ring index is the slow one; ICET_DESKEW_TIME_COLUMN_SLOW (i div period) + 0.5, period the
 *      rows per column.  s = (tau - t0) inv_span: the caller takes the reciprocal of the span once;
 *   4. d = s - s_ref, theta_a = d phi_a, u = (theta_x^2 + theta_y^2) + theta_z^2; unless u <= 1 the bits are copied, class out_of_range (more than one radian
 *      between the row and the reference instant; a NaN twist or parameter ends here, on the host and in HBM alike: it is never refused);
 *   5. A, B, C = the polynomials of degree 9 in u with the coefficients nearest to (-1)^k / (2k+1)!, / (2k+2)!, / (2k+3)!, by Horner from k = 9;
 *   6. sigma_a = d rho_a; c1 = theta x p, c2 = theta x c1, r1 = theta x sigma, r2 = theta x r1, each component two products and one difference,
 *      (a_y b_z - a_z b_y) and cyclic;
 *   7. out_a = (float)(((p_a + A c1_a) + B c2_a) + ((sigma_a + B r1_a) + C r2_a)), class moved.  s outside [0, 1] is extrapolated as it stands.
 * icet_deskew_device: n scans (HOST descriptors of DEVICE memory: src and dst N x 3 column-major float32 with leading dimensions ld and ld_out, 4-byte aligned,
 *   padding never read or written; dst == src with ld_out == ld is the in-place form) in ONE launch, asynchronous on the context's stream.  d_twists: NULL, or
 *   n x 6 DEVICE doubles that replace scans[k].twist; d_counts: NULL, or n DEVICE records, zeroed in stream order ahead of the launch.
 * icet_deskew: the same for HOST pointers inside the descriptors and HOST counts (may be NULL); staged, synchronous.
 * icet_deskew_twists_from_poses_device: d_twists[k] = scale log(T_k^-1 T_(k+1)), k = 0 .. n - 1, from n + 1 consecutive DEVICE float32 4 x 4 poses (what
 *   icet_pose_graph_optimize_device leaves in d_poses_out; the inverse of a pose is the transpose of its rotation), so that optimiser -> twists -> deskew ->
 *   icet_voxel_map_add_posed_device never leaves the device.  Valid for steps below 3 rad.  Asynchronous.
 * icet_twist_from_pose / icet_pose_from_twist (T = exp(s xi)): HOST only, no context, row-major 4 x 4 doubles.  icet_debug_deskew_rows: HOST only, the
 *   library's one compiled body of the rule over host arrays (x, y, z and out_x, out_y, out_z columns of n; time may be NULL outside array mode; cls n int32
 *   or NULL).
 * Refusals (ICET_ERR_BAD_ARG, the reason in icet_deskewer_last_error, nothing touched): a NULL handle or array, n < 0; a scan with n < 0, ld < n, ld_out < n
 *   or either >= 2^30; a NULL src or dst with n > 0, a NULL time in array mode with n > 0; a misaligned device pointer; an unknown mode, period <= 0 in a column
 *   mode; a dst that overlaps its src without being identical to it.  There is no CPU fall-back. */
#define ICET_DESKEW_TIME_ARRAY 0
#define ICET_DESKEW_TIME_COLUMN_FAST 1
#define ICET_DESKEW_TIME_COLUMN_SLOW 2
typedef struct icet_deskewer icet_deskewer;
typedef struct icet_deskew_scan {
    const float* src; int64_t n, ld;
    float* dst; int64_t ld_out;
    const float* time;            /* n floats, ICET_DESKEW_TIME_ARRAY only */
    int32_t time_mode, period;
    double t0, inv_span, s_ref;
    double twist[6];              /* rho | phi */
} icet_deskew_scan;               /* 128 bytes */
typedef struct icet_deskew_counts {
    int64_t moved, zero, nonfinite, bad_time, out_of_range, reserved[3];
} icet_deskew_counts;             /* 64 bytes */
icet_status icet_deskewer_create(icet_ctx* ctx, icet_deskewer** out);
icet_status icet_deskewer_destroy(icet_deskewer* h);
const char* icet_deskewer_last_error(const icet_deskewer* h);
icet_status icet_deskew_device(icet_deskewer* h, int32_t n, const icet_deskew_scan* scans, const double* d_twists, icet_deskew_counts* d_counts);
icet_status icet_deskew(icet_deskewer* h, int32_t n, const icet_deskew_scan* scans, icet_deskew_counts* counts);
icet_status icet_deskew_twists_from_poses_device(icet_deskewer* h, int32_t n, const float* d_poses, double scale, double* d_twists);
icet_status icet_twist_from_pose(const double T[16], double xi[6]);
icet_status icet_pose_from_twist(const double xi[6], double s, double T[16]);
icet_status icet_debug_deskew_rows(const icet_deskew_scan* motion, int64_t n, const float* x, const float* y, const float* z, const float* time,
                                   float* out_x, float* out_y, float* out_z, int32_t* cls);

/* Launch-shape and diagnostic knobs of ONE context (the library never reads the environment).  Defaults are the measured
 * optima.  Launch-shape knobs yield the same result bits; "force_exact", "guard_scale" and "lut_polar_quantile" preserve every
 * DECISION (the per-voxel counts n2_raw / n2_in) but move points between the 4-point runs and the runs of one, i.e. they regroup
 * float partial sums: X agrees to rounding, not bitwise.  Names: "lds_slots", "acc_pts",
 * "acc_blocks", "kf_pts", "rs_cap", "rs_max_cell" (0: per-bucket radix sort instead of the counting sort),
 * "keep" (the KEEP LIST of the point pass, batches of >= 32 pairs: H^T W H only sees scan-2 points in the angular bin of a voxel that has a scan-1 Gaussian -- src/icet.cpp:290-302 --
 * so a full pass also marks, per aligned group of 4 points, whether any of them is within an angular margin of such a bin, and later passes walk the list of marked
 * groups instead of the scan for as long as X stays within "keep_budget_t" (m, default 0.08) / "keep_budget_r" (Frobenius norm of the rotation difference, default 0.008)
 * of the X the marks were made at; a pair that leaves the budgets walks its whole scan once more and gets a new list.  The list pass forms the float partial sums of the
 * full pass exactly: SAME BITS with the option on, off, or with any budgets.  -1 / 1 on (default), 0 off; "keep_from" (default 1): first iteration whose pass makes marks),
 * "graph" (device-resident batches of <= 8 pairs: when a call's launch geometry and pointers equal the previous call's, the whole
 * solve is captured into a hipGraph and replayed from then on -- one hipGraphLaunch instead of ~33 launches on the host; 0 = never, default -1 = on),
 * "lds_rank" (the keyframe's stable multi-splits take a row's rank among equal classes from the value its LDS atomic hands back: -1 / 1 if
 * the device passed the order self-test run at icet_create, 0 = one ballot per class-id bit; same bits either way),
 * "packed_rows" (the keyframe's rank and row tables carry each row's voxel word in their spare bits, so the swap loop gathers it for run heads only and the voxel
 * split reads one word per position: -1, the default, whenever bits(largest scan 1 - 1) + bits(voxels - 1) + 2 <= 32 -- 75 x 24 with scans up to 2^19 rows,
 * 150 x 48 up to 2^17 --, 0 never, 1 required: a call whose shapes do not fit answers ICET_ERR_UNSUPPORTED; same bits either way),
 * "exec_bits_lds" (0: swap-loop bit table read from memory), "exec_pairwise" (which kernel computes the swap loop's executed-step bits:
 * 1 one block per pair from the recurrence, 0 chain walks over independent tiles, -1 by batch size), "fuse_solve" (batches below 32 pairs on grids up to 4096 voxels:
 * 1 the block of a pair that finishes its share of an iteration's point pass last runs the pair's solve in the same launch -- 7 launches less per solve, same
 * bits; default 0: measured no faster on MI355X, where a device-scope fence is an L2 write-back), "batch_parts" (0 = automatic), "batch_stage" (0..4), "force_exact"
 * (every scan-2 point through the literal classification), "library_sort" (0 only: the library has ONE sort, the
 * hand-written rank sort, and no build flag brings another; any other value answers ICET_ERR_UNSUPPORTED), "guard_scale" (>= 1), "lut_polar_quantile" (0..1), "snapshot_chunk_bytes" (payload bytes per chunk of icet_keyframe_store_save / _load; 0 = the default, 64 MiB), "pg_solver" (the pose-graph optimiser's linear solve: 0 conjugate gradients, the default; 1 the direct solve; 2 auto; any other value ICET_ERR_BAD_ARG), "map_lds" (icet_voxel_map_add_*: 1, the default, a block reduces its rows in LDS before it touches the table; 0 one global update per row; same contents), "map_query_prune" (icet_voxel_map_query_*: 1, the default, a block skips the queries whose run of x cells misses its chunk; 0 every cell is tested for every query; same bits), "map_evidence_prune" (icet_voxel_map_evidence_*: 1, the default, a block skips the scans whose run of x cells misses its chunk; same bits), "map_evidence_batch" (scans per batch of range images: 0, the default, as many as fit 64 MiB, else 1 .. 256; same bits), "map_snapshot_chunk_entries" (icet_voxel_map_save / _load: entries per chunk of the payload, 0 .. 2^30; 0, the default: 2^20; same bytes), "gn_cond_bound" (0 .. 1e6, default 2.5e5 -- a factor 4 below checkCondition's cutoff, because a float Cholesky inverse knows its own norm to a few per cent only at such condition numbers: an H^T W H whose Frobenius bound on
 * the condition number |A|_F |A^-1|_F exceeds it is inverted by the literal restatement of the reference's statements -- column-pivoted QR
 * pseudo-inverse, eigenvectors, pruning -- instead of a Cholesky factorisation; 0 = always literal.  Not a launch-shape knob: between the two
 * routes cov / dx differ by rounding times the condition number).  Unknown name or value
 * out of range: ICET_ERR_BAD_ARG. */
icet_status icet_set_option(icet_ctx* ctx, const char* name, double value);

/* The HIP stream (hipStream_t as void*) and device a context enqueues on -- for callers that produce scans on the GPU. */
void* icet_stream(icet_ctx* ctx);
int   icet_device(const icet_ctx* ctx);

/* --- the batched-pairs case over several GPUs of one node (BASELINE.json configs[3]) ---------
 * The reference has no counterpart: it constructs one ICET object per pair on the calling thread.  A handle owns one context and
 * one persistent host thread per device; pair k of a call runs on device_ids[k mod n_devices], and the 48 result floats per pair
 * are gathered into ONE buffer -- the caller's host arrays, or HBM of device_ids[0].  There is no data-path collective.  The
 * device-resident gather is, by option "gather": 0 (default) one strided peer copy per device over xGMI (peer access between
 * device_ids[0] and the others is enabled at create), or 1 ONE ncclAllGather over a communicator of the handle's devices (RCCL,
 * dlopen'ed on first use; needs distinct device ids) followed by the de-interleave on device_ids[0].  A process that runs one
 * rank per GPU gathers with torch.distributed / RCCL instead (icet_amd/dist.py). */
typedef struct icet_multi icet_multi;
icet_status icet_multi_create(icet_multi** handle, const int32_t* device_ids, int32_t n_devices);   /* each id < device count; an id may repeat (one context per ENTRY) */
icet_status icet_multi_destroy(icet_multi* handle);
const char* icet_multi_last_error(const icet_multi* handle);
int32_t     icet_multi_devices(const icet_multi* handle);
icet_ctx*   icet_multi_context(icet_multi* handle, int32_t i);      /* the context of device_ids[i] (e.g. for icet_reserve) */
/* "gather" (above), or any icet_set_option name, applied to every device's context. */
icet_status icet_multi_set_option(icet_multi* handle, const char* name, double value);
/* HOST pointers in and out, same meaning as icet_solve_batch. */
icet_status icet_multi_solve_batch(icet_multi* handle, const icet_params* p, int32_t n_pairs,
                                   const float* const* scan1, const int64_t* n1, const float* const* scan2, const int64_t* n2,
                                   const float* x0, float* x_out, float* pred_stds_out, float* cov_out);
/* Scans resident in HBM: scan1[k] / scan2[k] on device_ids[k mod n_devices]; d_x0 (n_pairs x 6 or NULL) and d_out (n_pairs x 48,
 * layout of icet_solve_batch_device) on device_ids[0].  Returns after the gather has completed (synchronous).  The devices'
 * streams are the handle's own: the scans, d_x0 and whatever last used d_out must have COMPLETED before the call -- or, for work
 * queued on one stream of device_ids[0], use the _after form: an event recorded on `producer_stream` (hipStream_t as void*, NULL =
 * none) when the call starts is waited for by every device's stream. */
icet_status icet_multi_solve_batch_device(icet_multi* handle, const icet_params* p, int32_t n_pairs,
                                          const icet_dev_scan* scan1, const icet_dev_scan* scan2, const float* d_x0, float* d_out);
icet_status icet_multi_solve_batch_device_after(icet_multi* handle, const icet_params* p, int32_t n_pairs,
                                                const icet_dev_scan* scan1, const icet_dev_scan* scan2, const float* d_x0, float* d_out,
                                                void* producer_stream);

/* The asynchronous form (review r3: the synchronous entry cost one process ~9 % against the stream-ordered single-context path, and eight
 * GPUs driven from one thread would start behind).  _async hands every device's share to its host thread and returns at once -- the
 * caller's descriptor arrays are copied, nothing waits for a device; calls queue up behind each other in order.  icet_multi_sync waits
 * until everything queued so far has completed on every device (d_out is then valid) and returns the first failure since the last sync.
 * producer_stream as in the _after form (NULL = none). */
icet_status icet_multi_solve_batch_device_async(icet_multi* handle, const icet_params* p, int32_t n_pairs,
                                                const icet_dev_scan* scan1, const icet_dev_scan* scan2, const float* d_x0, float* d_out,
                                                void* producer_stream);
icet_status icet_multi_sync(icet_multi* handle);

#ifdef __cplusplus
}
#endif
#endif /* ICET_HIP_H */
