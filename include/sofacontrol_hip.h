/*
 * sofacontrol_hip.h -- C ABI of libsofacontrol_hip.so (MI355X / gfx950).
 *
 * The reference (StanfordASL/soft-robot-control) is pure Python and has no FFI of its own: the seam
 * is its duck-typed Python protocol.  Each entry point below names the reference
 * method it serves (file:line relative to the reference root); the Python host package
 * (soft-robot-control_amd/sofacontrol_amd) binds these with ctypes and re-exposes the reference's
 * class/method surface.  INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error (SRH_E*); never throws; srh_last_error() gives
 *    the message of the last failure on the calling thread;
 *  - all arithmetic is IEEE float64 (the reference is numpy float64 throughout);
 *  - matrices are dense row-major; "ld" arguments are leading dimensions in elements;
 *  - `*_dev` entry points take DEVICE pointers (HBM) and a hipStream_t passed as void* (NULL = the
 *    null stream) and are asynchronous on that stream; entry points without the suffix take HOST
 *    pointers, stage through HBM and are synchronous on return;
 *  - handles are owned by the caller and are not thread-safe (one host thread per handle, as the
 *    reference's single SOFA/solver thread).
 */
#ifndef SOFACONTROL_HIP_H
#define SOFACONTROL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRH_OK        0
#define SRH_EINVAL   -1   /* bad argument (the reference raises RuntimeError / AssertionError)        */
#define SRH_EHIP     -2   /* HIP runtime error (no device, launch failure, ...)                      */
#define SRH_ENOMEM   -3
#define SRH_ENUMERIC -4   /* numerical failure (non-PD matrix, QP not solved: reference returns flags) */

const char *srh_last_error(void);
int srh_version(void);

/* ---- device plumbing (lets a host without torch stage buffers; not part of the reference) ---- */
int srh_device_count(int *count);
int srh_set_device(int device);
int srh_malloc(void **dptr, size_t bytes);
int srh_free(void *dptr);
int srh_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int srh_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int srh_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes);
int srh_memset(void *dptr, int value, size_t bytes);
int srh_sync(void);
/* The host-pointer entry points keep the device blocks they release in a size-class cache (<= 2 GiB per process)
 * instead of paying hipMalloc / hipFree per call -- hipFree waits for EVERY stream of the device, which would stall the
 * caller behind an asynchronous solver request; this returns the cached blocks to the driver. */
int srh_release_cached(void);
/* average duration in milliseconds of `iters` back-to-back launches are measured by the caller with
 * these (hipEvent on the given stream): */
int srh_event_create(void **ev);
int srh_event_destroy(void *ev);
int srh_event_record(void *ev, void *stream);
int srh_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms);   /* synchronises ev_stop */

/* =====================================================================================================
 * POD reduced-order map.          reference: sofacontrol/mor/pod.py
 * ===================================================================================================== */
typedef struct srom srom_t;

/* POD.__init__ (pod.py:14-20): U (n_f x r) row-major, q_ref / v_ref (n_f,) or NULL (= zeros).
 * Copies the basis to HBM and packs it into MFMA fragment order. */
int srom_create(srom_t **h, const double *U, int64_t n_f, int r, const double *q_ref, const double *v_ref);
int srom_destroy(srom_t *h);
int srom_dims(const srom_t *h, int64_t *n_f, int *r);

#define SROM_Q 0   /* U^T (qf - q_ref)      pod.py:46-47 */
#define SROM_V 1   /* U^T (vf - v_ref)      pod.py:48-49 */
#define SROM_X 2   /* V^T (xf - x_ref), x = [v; q], V = kron(I2, U)   pod.py:51-52 */
#define SROM_RAW 3 /* U^T m (no reference subtracted): rows of a matrix, pod.py:68-72 */

/* POD.compute_RO_state (pod.py:39-54), batched: X is (B x n_f) [SROM_Q/V/RAW] or (B x 2 n_f) [SROM_X],
 * one snapshot per row (the layout of np.asarray(data['q']), pod.py:149); out is (B x r) or (B x 2r). */
int srom_project(srom_t *h, int which, const double *X, int64_t B, double *out);
int srom_project_dev(srom_t *h, int which, const double *X_dev, int64_t B, int64_t ldx,
                     double *out_dev, int64_t ldo, void *stream);
/* utils.qv2x (sofacontrol/utils.py:129-130) on resident reduced coordinates: x (B x 2r, row pitch ldx) = [v ; q] from
 * q_dev (B x r, pitch ldq) and v_dev (B x r, pitch ldv; NULL: zero velocities) -- what the controllers do with the two
 * halves of compute_RO_state before the model / solver sees a reduced state (tpwl/controllers.py:96). */
int srom_qv2x_dev(const double *q_dev, int64_t ldq, const double *v_dev, int64_t ldv, int64_t B, int r,
                  double *x_dev, int64_t ldx, void *stream);

/* POD.compute_FO_state (pod.py:22-37), batched: Xr (B x r | B x 2r) -> out (B x n_f | B x 2 n_f). */
int srom_lift(srom_t *h, int which, const double *Xr, int64_t B, double *out);
int srom_lift_dev(srom_t *h, int which, const double *Xr_dev, int64_t B, int64_t ldr,
                  double *out_dev, int64_t ldo, void *stream);

/* POD.compute_RO_matrix (pod.py:56-72) for a dense row-major M (n_f x ncols):
 *   left && right (or neither): U^T M U (r x r), needs ncols == n_f
 *   left only : U^T M (r x ncols)           right only: M U (n_f x r), needs ncols == n_f */
int srom_reduce_matrix(srom_t *h, const double *M, int64_t ncols, int left, int right, double *out);
int srom_reduce_matrix_dev(srom_t *h, const double *M_dev, int64_t ncols, int left, int right,
                           double *out_dev, void *stream);
/* The same U^T M U for `count` dense n_f x n_f matrices in one call: TPWLSnapshotData.add_point reduces K, D, M and S of one
 * linearisation point back to back (tpwl/tpwl_utils.py:96-103 -> pod.py:56-72); groups of four share ONE launch pair.  M / out:
 * arrays of `count` pointers (row-major n_f x n_f in, r x r out). */
int srom_reduce_matrices(srom_t *h, const double *const *M, int count, double *const *out);
int srom_reduce_matrices_dev(srom_t *h, const double *const *M_dev, int count, double *const *out_dev, void *stream);

/* Snapshot Gramian G = S S^T, S (n_s x n_f) row-major, G (n_s x n_s): the method-of-snapshots route
 * to compute_POD (pod.py:181-200: sigma_i = sqrt(eig_i(G)), U = S^T W Sigma^-1).  With S sharded by
 * columns over ranks the partial Gramians are summed by an RCCL all-reduce in the host layer. */
int srom_gramian_dev(const double *S_dev, int64_t n_s, int64_t n_f, int64_t lds, double *G_dev,
                     void *stream);
int srom_gramian(const double *S, int64_t n_s, int64_t n_f, double *G);
/* The launch srom_gramian_dev makes for this shape on a card of `cus` compute units (cus <= 0: ask the current device; with
 * cus > 0 a host function, no GPU needed): ntile = 128 x 128 tiles per side (only the ntile (ntile + 1) / 2 on or above the
 * diagonal are computed), nfull = tiles computed whole, ntail = tiles of a partial last round that are split ksplit ways
 * along K and summed in part order (0: none, ksplit = 1); nfull + ntail = all tiles.  Any output pointer may be NULL. */
int srom_gramian_plan(int64_t n_s, int64_t n_f, int cus, int *ntile, int *nfull, int *ntail, int *ksplit);
/* process_snapshots (pod.py:157-178) on a resident snapshot matrix S (n_s x n_f, one snapshot per row, row pitch lds >= n_f).
 * Column statistics over the snapshots (each output n_f doubles on the device, any of them may be NULL):
 * min / max for 'normalize' (pod.py:165), mean for 'substract_mean' (pod.py:168). */
int srom_snapshot_stats_dev(const double *S_dev, int64_t n_s, int64_t n_f, int64_t lds, double *min_dev, double *max_dev,
                            double *mean_dev, void *stream);
/* 'normalize' in place: S <- (S - min) / (max + 1e-15 - min)   (pod.py:165) */
int srom_snapshot_normalize_dev(double *S_dev, int64_t n_s, int64_t n_f, int64_t lds, const double *min_dev,
                                const double *max_dev, void *stream);
/* 'substract_mean' in place: S <- S - mean   (pod.py:168) */
int srom_snapshot_center_dev(double *S_dev, int64_t n_s, int64_t n_f, int64_t lds, const double *mean_dev, void *stream);
/* 'clustering' (pod.py:170-174 -> compute_kmeans_centroids, pod.py:207-216: sklearn KMeans(k, n_init=100, max_iter=1000,
 * random_state=0)); the estimator's dense Lloyd algorithm restated on the device, one run from given centres:
 * C_dev (k x n_f) holds the initial centres and receives the final ones; labels_dev (n_s int32); tol = the absolute
 * threshold on the summed squared centre shift (sklearn: 1e-4 * mean column variance); *iters_out = Lloyd iterations.
 * srom_row_sqnorms_dev / srom_sqdist_rows_dev provide what the k-means++ seeding needs: |x_i|^2 and the squared
 * distances max(0, |y_c|^2 - 2 y_c . x_i + |x_i|^2) of every snapshot to nc given rows Y (nc x n_f) -> out (nc x n_s);
 * the seeding's random draws stay with the caller (numpy's RandomState in the reference's stack). */
int srom_row_sqnorms_dev(const double *S_dev, int64_t n_s, int64_t n_f, int64_t lds, double *out_dev, void *stream);
int srom_sqdist_rows_dev(const double *S_dev, int64_t n_s, int64_t n_f, int64_t lds, const double *Y_dev, int nc,
                         const double *xnorm_dev, double *out_dev, void *stream);
int srom_kmeans_lloyd_dev(const double *S_dev, int64_t n_s, int64_t n_f, int64_t lds, int k, double *C_dev, int max_iter,
                          double tol, int32_t *labels_dev, double *inertia_out, int *iters_out, void *stream);
/* eigh of the (symmetric) Gramian in place on the device (cyclic Jacobi kernels up to n = 2048, rocSOLVER dsyevd
 * above): on return row j of G_dev is
 * the eigenvector of the j-th smallest eigenvalue, w_dev (n) ascending.  Replaces the SVD of pod.py:190.
 * n <= 128: a Gramian whose null space stalls the sweeps (rank far below n) is finished with the pairs of its null cluster --
 * entries at or below n eps |diag| -- left alone; eigenvalues there are rounding noise of either sign. */
int srom_eigh_dev(double *G_dev, int64_t n, double *w_dev, void *stream);
/* The k LARGEST eigenpairs of the symmetric positive semidefinite G (n x n, left untouched) by blocked subspace iteration +
 * Rayleigh-Ritz (block = k + oversample <= 128; oversample < 0: max(16, k / 2)) -- what compute_POD keeps of the SVD
 * (pod.py:190-200) without the other n - k singular values: w_dev (k) descending; Wk_dev (n x k) = eigenvector columns
 * scaled by 1 / sqrt(w_i) (the input of srom_modes_dev) or NULL; Vt_dev (k x n) = eigenvector rows or NULL; *trace_out
 * = trace(G) (the truncation rule's denominator: tail energy = trace - sum w); *iters_out = subspace iterations until the
 * leading k eigenvalues settled to 1e-13 (<= 30), or 31 when they did not (no gap behind the block: take srom_eigh_dev).
 * k beyond the numerical rank: a column of Wk whose w_i <= 1e-28 w_0 or w_i <= 0 is zero (no division by a vanished sigma). */
int srom_eigh_topk_dev(const double *G_dev, int64_t n, int k, int oversample, double *w_dev, double *Wk_dev,
                       double *Vt_dev, double *trace_out, int *iters_out, void *stream);
/* W_k (n x k, row-major) = the k leading eigenvectors as columns, scaled by 1/sigma_i = 1/sqrt(w_i); V_dev, w_dev as
 * srom_eigh_dev leaves them (eigenvector rows, w ascending).  k beyond the numerical rank: a column whose w_i lies at or below
 * the rounding noise of the eigensolver, w_i <= max(1e-28, n eps) w_max, or w_i <= 0, is zero, and so is that column of
 * U = S^T W_k (no inf / NaN from a vanished sigma, no mode made of noise). */
int srom_select_modes_dev(const double *V_dev, const double *w_dev, int64_t n, int k, double *Wk_dev,
                          void *stream);
/* U_k = S^T W_k  (n_f x k) for eigenvector columns W_k (n_s x k, already scaled by 1/sigma).  Needs 0 < k <= 64, n_s > 0,
 * n_f > 0 and a row pitch lds >= n_f of S. */
int srom_modes_dev(const double *S_dev, int64_t n_s, int64_t n_f, int64_t lds, const double *W_dev,
                   int k, double *U_dev, void *stream);

/* =====================================================================================================
 * TPWL piecewise-affine model.    reference: sofacontrol/tpwl/tpwl.py, sofacontrol/scp/models/tpwl.py
 * ===================================================================================================== */
typedef struct stpwl stpwl_t;

/* Tables of the P linearisation points (tpwl.py:20-41; keys 'q','v','u','A_c','B_c','d_c' of the
 * tpwl_dict), reduced state x = [v; q], n_x = 2 r.  A_d/B_d/d_d are the pre-discretised tables
 * (TPWLATV.pre_discretize, tpwl.py:299-322) or NULL.  w_q, w_v = dist_weights (tpwl.py:165-166). */
int stpwl_create(stpwl_t **h, int P, int r, int n_u,
                 const double *q, const double *v, const double *u,
                 const double *A_c, const double *B_c, const double *d_c,
                 const double *A_d, const double *B_d, const double *d_d,
                 double w_q, double w_v);
int stpwl_destroy(stpwl_t *h);
/* install / replace the discrete tables (pre_discretize with another dt) */
int stpwl_set_discrete(stpwl_t *h, const double *A_d, const double *B_d, const double *d_d);
/* output model z = H x + z_ref (TPWL.set_output_model, tpwl.py:86-89); H (n_z x n_x) */
int stpwl_set_output(stpwl_t *h, const double *H, const double *z_ref, int n_z);

/* TPWL.calc_nearest_point (tpwl.py:160-168) for B states X (B x n_x): idx (B,) int32 */
int stpwl_nearest(stpwl_t *h, const double *X, int64_t B, int32_t *idx);
int stpwl_nearest_dev(stpwl_t *h, const double *X_dev, int64_t B, int32_t *idx_dev, void *stream);
/* The same search as the GuSTO kernels run it over the states of a horizon (tpwl::nearest_many, csrc/tpwl_dev.h): ONE workgroup of
 * `threads` (256 or 512) for `count` >= 1 states X (count x n_x) -> idx (count,).  With w_v = 0, P <= 64, r <= 32 and at least two
 * rounds of the workgroup's waves (count >= 2 threads / 64) the point table is held in registers; otherwise the wave search of
 * stpwl_nearest.  Same indices either way.  For tests and records. */
int stpwl_nearest_many(stpwl_t *h, const double *X, int count, int threads, int32_t *idx);
/* TPWLATV.get_jacobians, nn branch (tpwl.py:251-265): gathers (A,B,d)[idx] of the discrete
 * (discrete=1) or continuous tables: A (B x n_x x n_x), Bm (B x n_x x n_u), d (B x n_x) */
int stpwl_linearize(stpwl_t *h, const double *X, int64_t B, int discrete, double *A, double *Bm,
                    double *d, int32_t *idx);
/* TPWL.calc_weighting_factors (tpwl.py:170-191): W (B x P) softmin weights exp(-beta d_i / d_min),
 * normalised; one-hot at the first minimum when d_min == 0 */
int stpwl_weights(stpwl_t *h, const double *X, int64_t B, double beta, double *W);
/* TPWLATV.get_jacobians, weighting branch (tpwl.py:244-248): continuous A = sum_i w_i A_c[i] etc.;
 * W (B x P) optional output of the weights */
int stpwl_linearize_weighted(stpwl_t *h, const double *X, int64_t B, double beta, double *A, double *Bm,
                             double *d, double *W);
/* TPWL.discretize_dynamics (tpwl.py:272-297; zoh: sofacontrol/utils.py:302-335 zoh_affine) for `batch` continuous affine models
 * xdot = A x + B u + d at once: the stored points of pre_discretize (tpwl.py:299-322), the blended model of weighting-mode TPWL
 * (tpwl.py:244-250).  method: 0 fe, 1 be, 2 bil, 3 zoh.  A (batch x n x n), B (batch x n x m), d (batch x n) -> same shapes.
 * SRH_ENUMERIC if a model's I - c A is singular ("singular matrix (model i)"), and, for be, bil and zoh, if A, B or d of a model
 * holds a NaN or an Inf anywhere ("non-finite model (model i)": tested on the inputs as they are loaded, so it takes precedence over
 * "singular" for that model); i is the lowest failing index of the batch, the models that did not fail are written, the failed ones'
 * outputs are left untouched.  fe is elementwise, as the reference is: non-finite entries pass through and the call returns SRH_OK. */
int stpwl_discretize(int method, int n, int m, int64_t batch, const double *A, const double *B, const double *d, double dt,
                     double *Ad, double *Bd, double *dd);
int stpwl_discretize_dev(int method, int n, int m, int64_t batch, const double *A_dev, const double *B_dev, const double *d_dev,
                         double dt, double *Ad_dev, double *Bd_dev, double *dd_dev, void *stream);
/* TPWL.rollout (tpwl.py:193-216) for `batch` independent rollouts:
 * x0 (batch x n_x), U (batch x N x n_u) -> X (batch x (N+1) x n_x), Z (batch x (N+1) x n_z) or NULL */
int stpwl_rollout(stpwl_t *h, const double *x0, const double *U, int N, int64_t batch, double *X,
                  double *Z);
/* the same on resident buffers, asynchronous on `stream` (Z_dev may be NULL): the zero-input initial guess of a
 * receding-horizon solve (scp/ros.py:78-79) without leaving the device */
int stpwl_rollout_dev(stpwl_t *h, const double *x0_dev, const double *U_dev, int N, int64_t batch,
                      double *X_dev, double *Z_dev, void *stream);
/* The kernel a rollout of N stages and `batch` rollouts of this handle launches (a host function).  staged: 1 the region's panel
 * [A_d^T | B_d^T | d_d] stays in LDS and is reloaded when the nearest point changes, 0 the plain kernel that reads it from L2 at every
 * stage (layouts above 64 KB of LDS, n_x > 82 at n_u = 4; or a handle created under SRH_TPWL_ROLLOUT_PLAIN=1).  held: 1 the point
 * table sits in registers of one wave (staged, w_v = 0, P <= 64, r <= 32), 0 the general nearest-point search.  lds_bytes: the dynamic
 * LDS of the launch.  Both kernels give the same X and Z bit for bit.  Any output may be NULL. */
int stpwl_rollout_plan(stpwl_t *h, int N, int64_t batch, int *staged, int *held, size_t *lds_bytes);
/* TPWLGuSTO.get_characteristic_vals (scp/models/tpwl.py:66-84): x_char, f_char (n_x,) */
int stpwl_characteristic(stpwl_t *h, double *x_char, double *f_char);

/* =====================================================================================================
 * Discrete EKF over the TPWL model.                        reference: sofacontrol/tpwl/observer.py:33-126
 * State estimate x (n_x) and covariance Sigma (n_x x n_x) stay resident in HBM between steps.
 * ===================================================================================================== */
typedef struct sekf sekf_t;
/* DiscreteEKFObserver.__init__ (observer.py:52-67): C (n_y x n_x) reduced measurement matrix, y_ref (n_y)
 * or NULL, Sigma0 / W (n_x x n_x), V (n_y x n_y).  The model handle must outlive the filter. */
int sekf_create(sekf_t **out, stpwl_t *model, const double *C, const double *y_ref, int n_y,
                const double *Sigma0, const double *W, const double *V);
int sekf_destroy(sekf_t *h);
/* The dispatch of sekf_create as a pure host function (no GPU is initialised): which kernel a filter of n_x states and
 * n_y measurements runs.  path: 0 refused (bad sizes, or the step does not fit the 160 KB LDS), 1 VALU (ekf_kernel),
 * 2 MFMA generic (ekf_mfma_kernel<0>), 3 MFMA n_x = 60 (ekf_mfma_kernel<60>), 4 wide (ekf_wide_kernel).  lds_bytes: the
 * dynamic LDS of the launch (for the VALU layout with the largest n_u a model can have, 16; 0 when refused).  gain_form:
 * 0 Gauss-Jordan elimination on all waves (paths 2 to 4: a shape is put there only if the elimination fits it), 1 one-wave
 * Cholesky (path 1).  Honours SRH_EKF_NO_MFMA.  Any output may be NULL. */
int sekf_plan(int n_x, int n_y, int *path, size_t *lds_bytes, int *gain_form);
/* the same for a live handle: what sekf_create decided (with the model's own n_u) */
int sekf_handle_plan(sekf_t *h, int *path, size_t *lds_bytes, int *gain_form);
/* initialize (observer.py:76-86): overwrite the estimate and/or the covariance (either may be NULL) */
int sekf_set_state(sekf_t *h, const double *x, const double *Sigma);
int sekf_get_state(sekf_t *h, double *x, double *Sigma);
/* update = predict_state + update_state (observer.py:88-126).  u (n_u) != NULL runs the predictor with the
 * nearest-point discrete tables of the model, or with (A_d, B_d, d_d) when given (weighting-mode models);
 * y (n_y, full-order measurement, y_ref is subtracted) != NULL runs the filter update.  x_out (n_x) optional.
 * Returns SRH_ENUMERIC when the innovation covariance is not positive definite. */
int sekf_step(sekf_t *h, const double *u, const double *y, const double *A_d, const double *B_d,
              const double *d_d, double *x_out);
/* One call for the per-simulation-step path of a closed-loop controller (closed_loop_controller.py:205-233,
 * tpwl/controllers.py:128-157: compute_RO_state(xf=x) followed by observer.update(u_prev, y, dt)): the full-order
 * state x_full = [v_f; q_f] (2 n_f) is projected to x_reduced_out (2 r) on a side stream while the filter step
 * (sekf_step with the model's own discrete tables) runs on stream 0; both go through their pinned mirrors and the
 * host waits once for each.  x_hat_out (n_x) optional.  Errors as sekf_step / srom_project. */
int sekf_step_projected(sekf_t *h, srom_t *rom, const double *x_full, const double *u, const double *y,
                        double *x_reduced_out, double *x_hat_out);

/* `batch` filters over one model, stepped by one launch (workgroup b is filter b; the kernels are those of sekf_step, chosen by the
 * same rule: sekf_plan).  C, y_ref, W, V and the model's tables are shared by all filters; the estimate x (batch x n_x), the covariance
 * Sigma (batch x n_x x n_x) and a status word (batch int32: 0, or 1 after a step whose innovation covariance was not positive definite)
 * are per filter and resident.  Each predictor takes the table point nearest to its own filter's estimate.  Nearest-point models only:
 * the explicit (A_d, B_d, d_d) form of sekf_step is not batched.  Sigma0 (n_x x n_x) is installed in every filter, the estimates start
 * at zero.  Limits (SRH_EINVAL, the message names the one missed): batch >= 1, 0 < n_y <= n_x, a shape sekf_plan does not refuse.
 * The model handle must outlive the filters. */
typedef struct sekf_batch sekf_batch_t;
int sekf_batch_create(sekf_batch_t **out, stpwl_t *model, const double *C, const double *y_ref, int n_y,
                      const double *Sigma0, const double *W, const double *V, int64_t batch);
int sekf_batch_destroy(sekf_batch_t *h);
/* what sekf_batch_create decided (as sekf_handle_plan) and the number of filters.  Any output may be NULL. */
int sekf_batch_plan(sekf_batch_t *h, int *path, size_t *lds_bytes, int *gain_form, int64_t *batch);
/* overwrite the estimates x (batch x n_x) and/or the covariances Sigma (batch x n_x x n_x); either may be NULL */
int sekf_batch_set_state(sekf_batch_t *h, const double *x, const double *Sigma);
/* x (batch x n_x), Sigma (batch x n_x x n_x), status (batch int32: of each filter's last step); any may be NULL */
int sekf_batch_get_state(sekf_batch_t *h, double *x, double *Sigma, int *status);
/* idx (batch int32): the table point each filter's last predictor took (the one nearest to its own estimate); -1 before the first */
int sekf_batch_last_points(sekf_batch_t *h, int32_t *idx);
/* sekf_step for every filter: u (batch x n_u) != NULL runs the predictors (the model must be pre-discretised: SRH_EINVAL otherwise),
 * y (batch x n_y) != NULL the updates.  One upload through a pinned block, one launch, one copy back, one host wait.  A filter whose
 * innovation covariance is not positive definite sets its status word and keeps its x and Sigma; the others are unaffected.  x_out
 * (batch x n_x, optional) receives the resident estimate of every filter in either case.  Returns SRH_ENUMERIC when any filter
 * failed (the message counts them and names the first). */
int sekf_batch_step(sekf_batch_t *h, const double *u, const double *y, double *x_out);

/* Polyhedron(with_reproject=True).project_to_polyhedron (utils.py:364-407; the measurement re-projection of
 * SSM/controllers.py:96-97): Euclidean projection of `batch` points X (batch x n) onto {p : A p <= b}, A (n_rows x n)
 * row-major, n <= 16, n_rows <= 64 (the reference hands the same QP to OSQP).  An interior point finds the active set, an
 * active-set step on it returns the point: a returned point carries a KKT certificate (max(A p - b) <= 1e-12 scale,
 * multipliers >= -1e-12 scale, stationary and complementary by construction), scale = max(1, |x|_inf, |b|_inf), and is within
 * 1e-9 scale of the projection whatever its margin; the floor of scale at 1 makes that absolute for polyhedra smaller than 1.
 * Points with max(A x - b) <= 0 are returned bit for bit.  SRH_ENUMERIC, naming the first such point, when a point is not
 * finite or no certified point is found in 60 iterations (empty set); SRH_EINVAL for a non-finite A or b. */
int spoly_project(const double *A, const double *b, int n_rows, int n, const double *X, int64_t batch, double *out);
/* The same projection with a status word per point instead of a failed call -- the form the closed-loop advance kernels use on every
 * measurement (one device function, csrc/poly_dev.h: a point has the same bits here, in spoly_project and inside a loop):
 *    0  already inside (max(A x - b) > 0 is false): out = x bit for bit        1  projected, with the certificate above
 *   -1  no certified projection in 60 iterations (an empty polyhedron): out = x    -2  the point is not finite: out = x
 * SRH_EINVAL only for the shape limits and a non-finite A or b. */
int spoly_project_status(const double *A, const double *b, int n_rows, int n, const double *X, int64_t batch, double *out, int32_t *status);

/* =====================================================================================================
 * SSM polynomial reduced model.                                  reference: sofacontrol/SSM/ssm.py
 * f(x,u) = r_coeff phi_rom(x) + B u;  z = w_coeff phi_ssm(x) + z_ref;  x = v_coeff phi_ssm(z - z_ref),
 * phi = monomials of degree 1..order, graded, lexicographic with x1 first (get_poly_basis, ssm.py:158-164).
 * ===================================================================================================== */
typedef struct sssm sssm_t;
#define SSSM_CONT         0   /* continuous Jacobians (get_continuous_jacobians, ssm.py:198-204)        */
#define SSSM_FE           1   /* discretize_dynamics 'fe'  (ssm.py:279-283)                              */
#define SSSM_BE           2   /* 'be'  (ssm.py:285-289)                                                  */
#define SSSM_BIL          3   /* 'bil' (ssm.py:291-296)                                                  */
#define SSSM_DISCRETE_MAP 4   /* self.discrete: Jacobians of rd_coeff phi + Bd u (ssm.py:206-218)        */
int sssm_num_monomials(int dim, int order);
int sssm_exponents(int dim, int order, int32_t *exps);            /* (n_mon x dim) exponent table */
/* SSM.__init__ (ssm.py:24-71): r_coeff (n_x x n_rom), B (n_x x n_u), rd_coeff / Bd or NULL, w_coeff
 * (n_o x n_ssm), v_coeff (n_x x n_ssm), z_ref (n_o); n_rom / n_ssm = sssm_num_monomials(n_x / n_o, order).
 * Limits (SRH_EINVAL): 0 < n_x <= 32; 0 < n_u <= n_x | 1 (n_x + 1 for even n_x, n_x for odd: the discretisation scratch);
 * 0 < rom_order, ssm_order <= 7 (the kernels keep order + 1 level offsets in eight slots); the bases must fit the 160 KB LDS. */
int sssm_create(sssm_t **out, int n_x, int n_u, int n_o, int rom_order, int ssm_order,
                const double *r_coeff, const double *B, const double *rd_coeff, const double *Bd,
                const double *w_coeff, const double *v_coeff, const double *z_ref);
int sssm_destroy(sssm_t *h);
/* bookkeeping performance matrix H (n_o x n_x) used by iLQR cost Hessians (ssm.py:69-70; zeros by default) */
int sssm_set_output(sssm_t *h, const double *H);
/* SSMDynamics.get_jacobians / get_continuous_jacobians / get_discrete_jacobians (ssm.py:198-218) for B
 * points: X (B x n_x), U (B x n_u) -> A (B x n_x x n_x), Bm (B x n_x x n_u), d (B x n_x).
 * SSSM_BE and SSSM_BIL form sep = inv(A_c) (A_d - I) (ssm.py:279-301; np.linalg.inv raises on a singular A_c): the downloaded results
 * are scanned on the host, and a non-finite value returns SRH_ENUMERIC with "singular" and the index of the first such problem in
 * the message (the outputs have been written; the other problems' entries are valid).  sssm_rollout scans X the same way.  The
 * device-resident paths -- silqr_solve_ssm and the GuSTO-SSM plan -- run the same discretisation inside their kernels and are NOT
 * covered by this check. */
int sssm_linearize(sssm_t *h, const double *X, const double *U, int64_t B, int mode, double dt,
                   double *A, double *Bm, double *d);
/* reduced_dynamics / reduced_dynamics_discrete (ssm.py:167-178): F (B x n_x) */
int sssm_dynamics(sssm_t *h, const double *X, const double *U, int64_t B, int discrete, double *F);
/* reduced_to_observed C_map (ssm.py:170-171) -> Z (B x n_o, WITHOUT z_ref) and/or get_observer_jacobians
 * (ssm.py:220-227): H (B x n_o x n_x), c = C(x) - H x (B x n_o).  Z or H may be NULL. */
int sssm_observe(sssm_t *h, const double *X, int64_t B, double *Z, double *H, double *c);
/* compute_RO_state (ssm.py:338-344): X = v_coeff phi(Z - z_ref) */
int sssm_reduce(sssm_t *h, const double *Z, int64_t B, double *X);
/* SSM.rollout (ssm.py:134-156) for `batch` rollouts: x0 (batch x n_x), U (batch x N x n_u) ->
 * X (batch x (N+1) x n_x), Z (batch x (N+1) x n_o, includes z_ref) or NULL */
int sssm_rollout(sssm_t *h, const double *x0, const double *U, int N, int64_t batch, int mode, double dt,
                 double *X, double *Z);
/* The same rollout on device arrays, asynchronous on `stream`: the one launch sssm_rollout makes, no copy, no wait and no scan of X
 * for non-finite states (sssm_rollout is this between its copies). */
int sssm_rollout_dev(sssm_t *h, const double *x0_dev, const double *U_dev, int N, int64_t batch, int mode, double dt, double *X_dev,
                     double *Z_dev, void *stream);

/* =====================================================================================================
 * Riccati recursions.             reference: sofacontrol/lqr/lqr.py, sofacontrol/lqr/traj_tracking_lqr.py
 * ===================================================================================================== */
/* TrajTrackingLQR.perform_dlqr_recursion (traj_tracking_lqr.py:18-48) for per-step (A_i, B_i),
 * i = 0..n-1 in forward time order, terminal P = Q: K (n x n_u x n_x), P (n+1 x n_x x n_x) or NULL. */
int sric_tvlqr(const double *A, const double *B, int n_steps, int n_x, int n_u, const double *Q,
               const double *R, double *K, double *P);
/* the same with the linearisation taken from a TPWL handle at the nominal states xbar (n x n_x) */
int sric_tvlqr_tpwl(stpwl_t *h, const double *xbar, int n_steps, const double *Q, const double *R,
                    double *K, double *P);
/* solve_riccati (lqr.py:6-21): fixed point until ||L - L_old||_F <= tol (reference: 1e-4);
 * `batch` independent (A,B) pairs share Q, R.  L (batch x n_u x n_x), P (batch x n_x x n_x).  SRH_ENUMERIC, naming the
 * first such problem, when R + B^T P B is not positive definite at some iteration (L, P are then left unwritten);
 * reaching max_iter is not an error (the reference has none): iters = max_iter. */
int sric_dare_fixed_point(const double *A, const double *B, int64_t batch, int n_x, int n_u,
                          const double *Q, const double *R, double tol, int max_iter, double *L,
                          double *P, int32_t *iters);
/* dare (lqr.py:24-31, scipy.linalg.solve_discrete_are in the reference; per TPWL point at the start-up of the scp
 * controller, tpwl/controllers.py:238-246): the stabilising solution by the structure-preserving doubling algorithm,
 * quadratic convergence (about a dozen steps).  Stops when max|H_k+1 - H_k| <= tol max|H_k+1|.  Same shapes as above;
 * iters = doubling steps.  SRH_ENUMERIC when R or R + B^T P B is not positive definite, I + G H is singular, or
 * max_iter steps do not converge. */
int sric_dare(const double *A, const double *B, int64_t batch, int n_x, int n_u, const double *Q, const double *R,
              double tol, int max_iter, double *L, double *P, int32_t *iters);
/* The same solver for a wide input block, 1 <= n_u <= 64 (sric_dare keeps its n_u <= 16): the Luenberger gain of the ROMPC
 * observer is dare(A_d^T, C^T, Q, R) (baselines/rompc/observer.py:27), whose "input" dimension is the measurement dimension.
 * Same arguments, doubling steps, stopping rule, shapes and SRH_ENUMERIC cases; R and R + B^T P B are factored by the whole
 * workgroup.  n_x as far as sric_dare goes (above 62 or so the five n x n slots move from LDS to the HBM workspace). */
int sric_dare_wide(const double *A, const double *B, int64_t batch, int n_x, int n_u, const double *Q, const double *R,
                   double tol, int max_iter, double *L, double *P, int32_t *iters);
/* CLQR (lqr.py:57-64: control.lqr, slycot's continuous Riccati solver, in the reference): the stabilising solution P of
 * A^T P + P A - P B R^-1 B^T P + Q = 0 and the gain K = -R^-1 B^T P, stated for u = +K x like every gain of this library
 * (control.lqr returns -K).  A Cayley transform with the shift gamma = 1.5 max(||A||_inf, 1e-3) brings the equation to the doubling
 * loop of sric_dare: same stopping rule, iters = doubling steps, same shapes, `batch` continuous (A, B) pairs under one (Q, R),
 * 1 <= n_u <= 16.  SRH_ENUMERIC, naming the first such problem, when R is not positive definite, when A - gamma I, the start's
 * second pivot matrix or I + G H is singular or a value is not finite, and when min(max_iter, 48) steps do not converge to a fixed
 * point whose closed loop A + B K is stable (a pair that is not stabilisable ends in one of the last two; convergence later than
 * step 48 would mean a stability margin below gamma 2^-45, which the rounding of the start cannot tell from none). */
int sric_care(const double *A, const double *B, int64_t batch, int n_x, int n_u, const double *Q, const double *R,
              double tol, int max_iter, double *K, double *P, int32_t *iters);

/* =====================================================================================================
 * iLQR.                          reference: sofacontrol/lqr/ilqr.py, sofacontrol/lqr/config.py
 * ===================================================================================================== */
typedef struct silqr_params {
    int    max_iter;          /* config.py:3   50  */
    double epsilon;           /* config.py:4   0.1 */
    double alpha0, alpha_scaling, improv_lb, improv_ub, alpha_min;   /* config.py:13-17 */
    int    counter_limit;     /* config.py:19  5   */
    double rho0, drho0, rho_scaling, rho_increase_fp, rho_max, rho_min;  /* config.py:25-30 */
    /* the four switches of config.py:6-9, 31 (all 1 in the reference's configuration):
     *   include_input_var_constraint  1: the input term of the cost is (u_t - u_{t-1})' R (u_t - u_{t-1}) (u_{-1} = u_last),
     *                                 0: u_t' R u_t                                          (ilqr.py:145-152, 250-256)
     *   do_linesearch                 0: the first forward pass (alpha0) is always accepted     (ilqr.py:75-88)
     *   regularize                    0: Q~_uu = Q_uu, Q~_ux = Q_ux; a Q_uu that is not positive definite ends the solve with
     *                                    iters = -1 (the reference prints a warning and goes on with the inverse of an
     *                                    indefinite matrix, ilqr.py:276-287)
     *   state_regularization          0: Q~_uu = Q_uu + rho I, Q~_ux = Q_ux                    (ilqr.py:264-270) */
    int    include_input_var_constraint, do_linesearch, regularize, state_regularization;
} silqr_params;
void silqr_default_params(silqr_params *p);

/* iLQR.ilqr_computation (ilqr.py:27-107) for `batch` independent problems on one TPWL model:
 *   x0 (batch x n_x), z_target (batch x (N+1) x n_z, absolute: includes z_ref), u_warm (batch x N x n_u)
 *   or NULL, u_last (batch x n_u) or NULL; Q, Qf (n_z x n_z), R (n_u x n_u).
 * Outputs x (batch x (N+1) x n_x), u (batch x N x n_u), K (batch x N x n_u x n_x), cost (batch),
 * iters (batch). */
int silqr_solve(stpwl_t *h, int N, int64_t batch, const double *x0, const double *z_target,
                const double *u_warm, const double *u_last, const double *Q, const double *R,
                const double *Qf, const silqr_params *p, double *x, double *u, double *K,
                double *cost, int32_t *iters);
/* The same on an SSM model: (A_t, B_t, d_t) = SSMDynamics.get_jacobians(x_t, u_t, dt) at every step of every
 * forward pass (ilqr.py:155), z = C_map(x) + z_ref in the costs, the model's constant H in the cost
 * Jacobians (ilqr.py:176-184).  mode = SSSM_FE / BE / BIL / DISCRETE_MAP. */
int silqr_solve_ssm(sssm_t *h, int mode, double dt, int N, int64_t batch, const double *x0,
                    const double *z_target, const double *u_warm, const double *u_last, const double *Q,
                    const double *R, const double *Qf, const silqr_params *p, double *x, double *u,
                    double *K, double *cost, int32_t *iters);

/* A resident iLQR plan: `batch` problems of horizon N on one pre-discretised TPWL model.  The handle owns every buffer silqr_solve
 * allocates per call -- inputs, x, u, K, cost, iters and the kernel's work space -- and launches the same kernel through the same
 * launcher, so a solve gives silqr_solve's results bit for bit while the policy (K above all: batch x N x n_u x n_x doubles) may stay
 * on the device.  Q, Qf (n_z x n_z), R (n_u x n_u); p NULL: silqr_default_params.  SSM models are not offered.  The model must outlive
 * the plan. */
typedef struct silqr_plan silqr_plan_t;
int silqr_plan_create(silqr_plan_t **out, stpwl_t *h, int N, int64_t batch, const double *Q, const double *R, const double *Qf,
                      const silqr_params *p);
int silqr_plan_destroy(silqr_plan_t *p);
/* z_target: shared != 0: ((N+1) x n_z), one block across PCIe, replicated for every problem on the device; shared == 0:
 * (batch x (N+1) x n_z).  Absolute, as silqr_solve's. */
int silqr_plan_set_target(silqr_plan_t *p, const double *z_target, int shared);
/* u_last (batch x n_u) of the solves that follow; NULL: none (zeros), as a NULL u_last of silqr_solve */
int silqr_plan_set_u_last(silqr_plan_t *p, const double *u_last);
/* One solve from host x0 (batch x n_x), u_warm (batch x N x n_u) or NULL, u_last (batch x n_u) or NULL (installed as by
 * silqr_plan_set_u_last).  Any output may be NULL: what is not asked for does not cross PCIe. */
int silqr_plan_solve(silqr_plan_t *p, const double *x0, const double *u_warm, const double *u_last, double *x, double *u, double *K,
                     double *cost, int32_t *iters);
/* The policy, cost and iterations of the last solve (host or device side); any may be NULL */
int silqr_plan_policy(silqr_plan_t *p, double *x, double *u, double *K, double *cost, int32_t *iters);
int silqr_plan_dims(silqr_plan_t *p, int *N, int *n_x, int *n_u, int *n_z, int64_t *batch);

/* =====================================================================================================
 * LOCP (the horizon QP) and GuSTO. reference: sofacontrol/scp/locp.py, sofacontrol/scp/gusto.py
 * ===================================================================================================== */
typedef struct slocp_problem {
    int N, n_x, n_u, n_z;
    const double *H;        /* (n_z x n_x)                          locp.py:29          */
    const double *Qz, *R;   /* (n_z x n_z), (n_u x n_u)             locp.py:30-31       */
    const double *Qzf;      /* (n_z x n_z) or NULL                  locp.py:32, 251-252 */
    const double *x_scale;  /* (n_x,) = 1/|x_char| or NULL (ones)   locp.py:47-51       */
    int nU;  const double *UA, *Ub;    /* U.A (nU x n_u), U.b       locp.py:300-303     */
    int nX;  const double *XA, *Xb;    /* X.A (nX x n_x), X.b       locp.py:330-333     */
    int nXf; const double *XfA, *Xfb;  /* terminal set              locp.py:336-337     */
    int ndU; const double *dUA, *dUb;  /* dU.A (ndU x n_u), dU.b    locp.py:305-308: must be 0 here -- the rate rows
                                        * couple consecutive stages; the host layer passes them as state rows of the
                                        * augmented state [x; u_prev; du] (sofacontrol_amd/scp/locp.py) */
    int tr_active;                     /* is_tr_active              locp.py:57          */
} slocp_problem;

/* LOCP.update + solve + get_solution (locp.py:98-203) for `batch` independent QPs of one shape:
 *   Ad (batch x N x n_x x n_x), Bd (batch x N x n_x x n_u), dd (batch x N x n_x), x0 (batch x n_x),
 *   xk (batch x (N+1) x n_x) trust-region centre, delta/omega (batch), z (batch x (N+1) x n_z) or NULL,
 *   zf (batch x n_z) or NULL, u_des (batch x N x n_u) or NULL.
 * Outputs x (batch x (N+1) x n_x), u (batch x N x n_u), s (batch x (N+1)), J (batch; objective value
 * without the 1/2, as cvxpy reports), status (batch; 0 = optimal, else the reference's `success=False`). */
int slocp_solve(const slocp_problem *prob, int64_t batch, const double *Ad, const double *Bd,
                const double *dd, const double *x0, const double *xk, const double *delta,
                const double *omega, const double *z, const double *zf, const double *u_des,
                double *x, double *u, double *s, double *J, int32_t *status, int32_t *iters);

/* The same QP with everything resident (round 3): constants, horizon buffers, work blocks and result buffers are created once
 * for a fixed batch and reused by every solve -- what the host loops around the device QP call once per SCP iteration
 * (GuSTO over SSM / weighting-mode models: scp/gusto.py:371-402; linear MPC: the LOCP of locp.py with is_tr_active=False).
 * slocp_plan_solve: host pointers as slocp_solve; Ad = Bd = dd = NULL keeps the horizon of the previous call resident
 * (LOCP.update(full=False), locp.py:139-141: only delta / omega / x0 change); xk, z, zf, u_des NULL keep theirs.
 * slocp_plan_solve_dev: every array already in HBM (the linearisation kernels' outputs can be passed straight in), results
 * written to device pointers, asynchronous on `stream`; s_dev / iters_dev may be NULL. */
typedef struct slocp_plan slocp_plan_t;
int slocp_plan_create(slocp_plan_t **out, const slocp_problem *prob, int64_t batch);
void slocp_plan_destroy(slocp_plan_t *plan);
int slocp_plan_solve(slocp_plan_t *plan, const double *Ad, const double *Bd, const double *dd, const double *x0,
                     const double *xk, const double *delta, const double *omega, const double *z, const double *zf,
                     const double *u_des, double *x, double *u, double *s, double *J, int32_t *status, int32_t *iters);
int slocp_plan_solve_dev(slocp_plan_t *plan, const double *Ad_dev, const double *Bd_dev, const double *dd_dev,
                         const double *x0_dev, const double *xk_dev, const double *delta_dev, const double *omega_dev,
                         const double *z_dev, const double *zf_dev, const double *ud_dev, double *x_dev, double *u_dev,
                         double *s_dev, double *J_dev, int32_t *status_dev, int32_t *iters_dev, void *stream);
/* The same with new_horizon = 0 for a horizon that has not changed since the previous call with the SAME Ad_dev / Bd_dev: the
 * transposed copies of that call are reused (slocp_plan_solve_dev transposes the whole batch x N horizon on every call). */
int slocp_plan_solve_dev_resident(slocp_plan_t *plan, int new_horizon, const double *Ad_dev, const double *Bd_dev,
                                  const double *dd_dev, const double *x0_dev, const double *xk_dev, const double *delta_dev,
                                  const double *omega_dev, const double *z_dev, const double *zf_dev, const double *ud_dev,
                                  double *x_dev, double *u_dev, double *s_dev, double *J_dev, int32_t *status_dev,
                                  int32_t *iters_dev, void *stream);

/* Which kernels a plan launches -- for tests and bench records (parity is claimed per instantiation; what ran is otherwise
 * visible only in a rocprof trace).  family: 1 = the lean condensed kernel first (csrc/lean.hip) with the fused kernel
 * (csrc/gusto.hip / scp.hip) taking what it hands over, 0 = the fused kernel alone.  lean_args = the template arguments of
 * the lean instantiation <n_u, n_x (0: run time), lanes per stage for the state rows (0: general row handling), horizon
 * (0: run time), first LDS-resident stage, state rows> (zeros when family = 0); fused_args = <split panel, n_u, n_x> of the
 * fused instantiation (0: that extent is a run-time value).  handed_over = problems (LOCP) / rollouts (GuSTO) of the LAST
 * solve that the lean kernel passed to the fused one (-1: no solve yet; 0 when family = 0).  The call waits for the plan's
 * last solve.  The instantiation is chosen when the plan is created. */
typedef struct srh_kernel_info {
    int32_t family;
    int32_t lean_args[6];
    int32_t fused_args[3];
    int32_t handed_over;
    int32_t lds_bytes_lean, lds_bytes_fused;
    int32_t threads;
} srh_kernel_info;
int slocp_plan_info(slocp_plan_t *plan, srh_kernel_info *info);

/* Whether QPs of this shape take the condensed (output-space) interior point for their trust-region-free pass
 * (csrc/locp_cond.h): enabled, the number of output directions found (rows of C_o spanning Cq, X.A, Xf.A) and whether
 * the input Hessian blocks 2R + U.A^T D U.A are diagonal for every D.  For tests and records. */
int slocp_condensed_info(const slocp_problem *prob, int *enabled, int *n_outputs, int *diag_input_hessian);

typedef struct sgusto_params {
    double delta0, omega0, rho, beta_fail, gamma_fail, epsilon, omega_max, convg_thresh; /* gusto.py:12-22 */
    int    max_gusto_iters;
} sgusto_params;
void sgusto_default_params(sgusto_params *p);
/* GuSTO's step rule (csrc/scp_types.h: what the kernels do with delta, omega and the previous accepted step after every QP) replayed on
 * the HOST over a script of T QP answers, each (md = max_k |x_scale (x_k - xbar_k)|_inf, J, rho_k, viol = largest state-constraint
 * violation, dsum = sum_k |x_scale (x_k - xbar_k)|_2); N, n_x as the convergence measure divides by them.  Needs no GPU; for tests of
 * the rule.  steps (T x 4): per iteration delta and omega of its QP, 1.0 if the step was accepted, J of the last accepted step after it;
 * iters = answers consumed (the rule may stop before T), status (0, 2 or 3 as sgusto_solve), converged. */
int sgusto_rule_replay(const sgusto_params *par, int N, int n_x, int T, const double *script, double *steps, int32_t *iters,
                       int32_t *status, int32_t *converged);

/* The interior point's rule on one inequality row (csrc/ipm_rule.h: the functions all seven QP kernels call) evaluated on the HOST, one
 * phase per call, over n rows.  rows (n x 8): g, t, lambda, rg, rc, dt, dlambda, a.d of each row (a phase reads what it needs); par (8)
 * and the results out (n x 8, columns as listed) and scal (8) per phase:
 *   INIT       par: unit weight                          out: D, rho, lambda
 *   COLD       par: min g, max g                         out: t, lambda                 scal: the shifts sh_t, sh_l
 *   WARM       par: poison (0 / 1); lambda = previous    out: t, lambda
 *   PRED       par: dreg                                 out: rg, D, rho, running sum lambda t, running max |rg|
 *   CORR       par: dreg, sigma, mu                      out: rc, rho
 *   DIRECTION  par: dreg, pred (0 / 1)                   out: dlambda, dt, the step bound of t, of lambda, running bound (from 1e300)
 *   AFFINE     par: amax, mu, row count                  out: the row's term at the affine step, running sum
 *                                                        scal: a_aff, a (the step taken from this amax), mu_aff, sigma
 *   ADVANCE    par: a                                    out: t, lambda
 *   SCALES     par: max |target gradient|, max |U.b|, omega, delta, reg (n = 0)         scal: scale_d, scale_p, dreg
 *   VERDICT    rows: ok (0 / 1), mu, rd, rp, iteration, row count; par: scale_d, scale_p, tol, max_iter, near_opt before the first row
 *              out: the predictor's verdict (a status, or -1 = go on; near_opt carries from row to row), near_opt after it, the
 *              verdict of a starting / corrector system with this ok, the verdict on this row count
 *   CONVERGED  rows: (unused), mu, rd, rp; par: scale_d, scale_p, tol
 *              out: 1.0 if the stopping test holds (ipm::converged), 1.0 if its part without rd holds (ipm::may_converge)
 * scal[7] = the warm-start floor in every phase.  Needs no GPU; for tests of the rule. */
enum { SQP_IPM_INIT = 0, SQP_IPM_COLD, SQP_IPM_WARM, SQP_IPM_PRED, SQP_IPM_CORR, SQP_IPM_DIRECTION, SQP_IPM_AFFINE, SQP_IPM_ADVANCE,
       SQP_IPM_SCALES, SQP_IPM_VERDICT, SQP_IPM_CONVERGED };
int sqp_ipm_rule_replay(int phase, int n, const double *rows, const double *par, double *out, double *scal);

/* The tile factorisation of K on one wave set of the lean kernels, as wave `wave` (0 .. 3) runs it: the ordered list of its events,
 * produced on the host by the roster functions the device code calls (which waves work in which tile row, their tiles, every counter
 * target).  K has KT x KT tiles of 16 x 16 (1 <= KT <= 8); wave 0 is the chain of diagonal factorisations, wave w >= 1 is worker w - 1.
 *   nwk0 = 3: the full-size workgroup's set, three workers in every row (code is ignored);
 *   nwk0 = 1: the half-size workgroup, whose waves 2 and 3 also run the front of the Newton solve.  code 0: the front only; code +k:
 *             the front, then workers in the rows k .. KT - 2; code -k: workers in the rows 0 .. k - 1, then the front (1 <= k <= KT - 2;
 *             any other code counts as 0).  *code_in_effect (may be NULL) receives the code used.
 * An event is four int32: {kind, a, b, c}.  WAIT: counter a has reached b; SIGNAL: counter a += 1 (counters: 0 trailing updates finished,
 * 1 diagonal inverses published, 2 panel tiles written, 3 early tiles of the next row); READ: tile (a, b); CHOL / PANEL / UPDATE: tile
 * (a, b) is rewritten by that operation of tile row c; FRONT: the front of the Newton solve.  At most `cap` events are written, *count
 * is the length of the whole list.  Needs no GPU; for tests of the protocol. */
enum { SLEAN_EV_WAIT = 0, SLEAN_EV_SIGNAL, SLEAN_EV_READ, SLEAN_EV_CHOL, SLEAN_EV_PANEL, SLEAN_EV_UPDATE, SLEAN_EV_FRONT };
int slean_roster_replay(int KT, int code, int nwk0, int wave, int cap, int32_t *events, int32_t *count, int32_t *code_in_effect);

/* y = G u of the half-size lean kernel (horizon NF, M inputs, NP = 2 NF <= 128 output columns) as lane `lane` (0 .. 63) of wave `wave`
 * of a wave set of `set_size` threads (128: the Newton front, 256: the whole workgroup) runs it, produced on the host by the schedule
 * functions the device code calls.  Column i of the packed G^T is summed in four chains, chain c over the stages c, c + 4, .. <= i / 2 of
 * every input in turn; a lane owns one (column, chain) task per round, the four tasks of a column sit in one quad of lanes.  A step is
 * nine int32 {round, input, step, column, chain, stage, flags, packed, toeplitz}, in the order the lane executes them: stage = the stage
 * whose term the step adds to the chain, or -1 where the lane is outside the triangle and adds nothing; packed / toeplitz = the index it
 * reads, in the packed rows / in the Toeplitz generators (M x NP) of a single-region G.  flags: SLEAN_GU_SPARE = the quad stands past
 * the round's last column (it repeats that column and stores nothing), SLEAN_GU_STORES = this lane stores the column's sum.  At most
 * `cap` steps are written, *count is the length of the whole list.  Needs no GPU; for tests of the schedule. */
enum { SLEAN_GU_SPARE = 1, SLEAN_GU_STORES = 2 };
int slean_gu_schedule(int NF, int M, int set_size, int wave, int lane, int cap, int32_t *steps, int32_t *count);

/* GuSTO.solve (gusto.py:283-487) on a pre-discretised nn-TPWL model, `batch` independent rollouts:
 *   x0 (batch x n_x), u_init (batch x N x n_u), x_init (batch x (N+1) x n_x), z (batch x (N+1) x n_z)
 *   or NULL, zf, u_des as slocp_solve; x_char / f_char (n_x,) or NULL (ones); dt = horizon step.
 * Outputs xopt (batch x (N+1) x n_x), uopt (batch x N x n_u), zopt (batch x (N+1) x n_z) = H xopt
 * (gusto.py:486), iters (batch) = number of SCP iterations (LOCP solves) performed,
 * status (batch; 0 ok, 1 = a QP could not be solved (gusto.py:357-365), 2 = omega > omega_max,
 * 3 = max iterations), trace (batch x max_trace x 4: J, delta, omega, rho_k per iteration) or NULL. */
int sgusto_solve(stpwl_t *h, const slocp_problem *prob, const sgusto_params *par, double dt,
                 int64_t batch, const double *x0, const double *u_init, const double *x_init,
                 const double *z, const double *zf, const double *u_des, const double *x_char,
                 const double *f_char, double *xopt, double *uopt, double *zopt, int32_t *iters,
                 int32_t *status, double *trace, int max_trace);

/* Resident form of sgusto_solve: the plan owns the device copies of the problem constants and the
 * per-rollout workspace for a fixed batch size, so that repeated receding-horizon solves (the
 * gusto_callback of scp/ros.py:94-127) launch ONE kernel and touch no host memory.  The `_dev` entry
 * point takes device pointers laid out as in sgusto_solve and is asynchronous on `stream`. */
typedef struct sgusto_plan sgusto_plan_t;
int sgusto_plan_create(sgusto_plan_t **plan, stpwl_t *h, const slocp_problem *prob, const sgusto_params *par,
                       double dt, int64_t batch, const double *x_char, const double *f_char, int max_trace);
int sgusto_plan_destroy(sgusto_plan_t *plan);
int sgusto_plan_set_max_iters(sgusto_plan_t *plan, int max_gusto_iters);   /* gusto.py:142-147 */
/* Solver state across solves (sofacontrol/scp/locp.py:181 `self.prob.solve(warm_start=self.warm_start, ...)`: the reference's cvxpy
 * problem object lives as long as the GuSTO object, so with warm_start=True its solver starts EVERY QP -- also the first one of the next
 * GuSTO.solve -- from the previous solution).  on = 1: the first QP of a solve starts from the minimiser and multipliers the same rollout's
 * previous solve ended with (lean kernels; later QPs of a solve always do).  Default 0: every solve starts cold (what bench.py times). */
int sgusto_plan_set_warm_across(sgusto_plan_t *plan, int on);
/* *active = 1 iff the flag above is set AND this plan's kernels honour it (lean kernels with the box-row interior point); fused-only
 * plans and general-row lean variants start every solve cold whatever was requested. */
int sgusto_plan_warm_across_active(const sgusto_plan_t *plan, int *active);
/* GuSTO on an SSM polynomial model (sofacontrol/scp/models/ssm.py + sofacontrol/SSM/ssm.py:198-235), the whole solve -- analytic
 * linearisation of the dynamics and of the output map along the trajectory, the LOCP QP with per-stage output maps (locp.py:231-245,
 * 312-329), the tests and the acceptance rules of gusto.py:371-473 -- inside ONE kernel launch per call: the loop the reference's
 * hardware driver runs every control period (examples/hardware/diamond_SSM.py:353-361).  `prob`: the QP in the augmented state
 * [x ; zeta] (n_x = n + n_o, H = [0 I], x_scale = 0 on zeta) when the model's output map is nonlinear, else the plain QP with the
 * constant H; `mode`: discretisation as sssm_linearize; Hm (n_z x n): model.H of zopt = H xopt (gusto.py:486); XA / Xb (nX x n): the state
 * polyhedron as GuSTO.state_constraints_violated applies it to the states (gusto.py:185-201), or NULL.  Arrays as sgusto_solve with
 * n_x = the model's n.  status: 0 ok, 1 a QP could not be solved, 2 omega > omega_max, 3 max iterations.
 * Input-rate rows (prob->ndU > 0: dUA (ndU x n_u), dUb; dU.A (u_{k+1} - u_k) <= dU.b, k = 0..N-2, locp.py:305-308) are taken where the
 * one-wave QP in the space of the inputs has room for them (sgusto_ssm_rate_rows_fit; not under SRH_GUSTO_SSM_NO_DENSE), refused
 * otherwise.  With them a rollout whose QP needs its trust-region rows -- the relaxed minimiser leaves the trust region, or the step
 * before it ended on its boundary and was rejected -- ends with status -78 (SSM_NEEDS_HOST), xopt / uopt = the initial trajectory:
 * the caller solves that rollout again by other means (GuSTO: the host loop); no rate row is ever dropped. */
typedef struct sgusto_ssm_plan sgusto_ssm_plan_t;
int sgusto_ssm_plan_create(sgusto_ssm_plan_t **plan, sssm_t *model, const slocp_problem *prob, const sgusto_params *par, double dt,
                           int mode, int64_t batch, const double *f_char, const double *Hm, int nX, const double *XA, const double *Xb,
                           int max_trace);
int sgusto_ssm_plan_destroy(sgusto_ssm_plan_t *plan);
/* Host arithmetic only (no GPU): *fits = 1 when a plan whose QP has these dimensions (n_x: the QP's state, the augmented one when the
 * outputs are carried) takes ndU rate rows -- N n_u <= 16, N (nU + nX) + (N - 1) ndU <= 64 rows, no terminal rows, a small model:
 * the rule of the dense one-wave QP (csrc/locp_dense_u.h: qdu::limit), which sgusto_ssm_plan_create applies.  ndU = 0: whether
 * that QP runs at all. */
int sgusto_ssm_rate_rows_fit(int N, int n_x, int n_u, int n_z, int nU, int nX, int nXf, int ndU, int *fits);
int sgusto_ssm_plan_set_max_iters(sgusto_ssm_plan_t *plan, int max_gusto_iters);
int sgusto_ssm_plan_set_warm_across(sgusto_ssm_plan_t *plan, int on);   /* as sgusto_plan_set_warm_across (locp.py:181) */
/* as sgusto_plan_warm_across_active: *active = 1 when warm_across was requested and the plan's shape runs the lean one-wave interior point
 * or the dense one-wave QP (the only routes that keep a rollout's solver state) */
int sgusto_ssm_plan_warm_across_active(const sgusto_ssm_plan_t *plan, int *active);
int sgusto_ssm_plan_solve(sgusto_ssm_plan_t *plan, const double *x0, const double *u_init, const double *x_init, const double *z,
                          const double *u_des, double *xopt, double *uopt, double *zopt, int32_t *iters, int32_t *status, double *trace);
int sgusto_ssm_plan_solve_dev(sgusto_ssm_plan_t *plan, const double *x0_dev, const double *u_init_dev, const double *x_init_dev,
                              const double *z_dev, const double *u_des_dev, double *xopt_dev, double *uopt_dev, double *zopt_dev,
                              int32_t *iters_dev, int32_t *status_dev, double *trace_dev, void *stream);
/* The shapes an SSM plan was created with (any output may be NULL): n_x = the MODEL's n (not the QP's augmented state), mode = the
 * discretisation of the plan's model, ndU = the rows of its rate polyhedron. */
int sgusto_ssm_plan_dims(const sgusto_ssm_plan_t *plan, int *N, int *n_x, int *n_u, int *n_z, int64_t *batch, double *dt, int *mode,
                         int *ndU);
/* As sgusto_plan_costs_dev: the LOCP value of the solution each rollout of the plan's LAST solve returned, copied device-to-device
 * into J_dev (batch) on `stream`, behind the solve enqueued there: no host wait. */
int sgusto_ssm_plan_costs_dev(sgusto_ssm_plan_t *plan, double *J_dev, void *stream);

/* Which kernel instantiation a solve of this plan launches: split (1: split W panel, n_x > 64), n_u_fixed / n_x_fixed
 * = the compile-time n_u / n_x of the instantiation (0: that extent is a run-time value; 0, 0 = the all-sizes
 * kernel).  For tests and bench records: parity is claimed per instantiation. */
int sgusto_plan_variant(const sgusto_plan_t *plan, int *split, int *n_u_fixed, int *n_x_fixed);
/* Optimal LOCP value of the solution each rollout of the plan's LAST solve returned (the cost `Jstar` of the last accepted
 * SCP step, gusto.py:340-370; +inf for a rollout that never accepted a step): J (batch).  What a sharded batch gathers to
 * pick its best rollout (distributed.gather_rollout_costs).  Waits for the solve. */
int sgusto_plan_costs(sgusto_plan_t *plan, double *J);
/* The same costs copied device-to-device into J_dev (batch) on `stream`, behind the solve enqueued there: no host wait. */
int sgusto_plan_costs_dev(sgusto_plan_t *plan, double *J_dev, void *stream);
/* The shapes a plan was created with (any output may be NULL); has_Qzf = 1 when the problem has a terminal cost (zf is read). */
int sgusto_plan_dims(const sgusto_plan_t *plan, int *N, int *n_x, int *n_u, int *n_z, int64_t *batch, double *dt, int *has_Qzf);
/* srh_kernel_info of a GuSTO plan (see slocp_plan_info). */
int sgusto_plan_info(sgusto_plan_t *plan, srh_kernel_info *info);
/* QPs of the plan's LAST solve that the lean kernel condensed by the single-region recursion (every stage of the horizon in
 * one TPWL region: the condensed matrix is block-Toeplitz and is built from one chain of N products); 0 for a plan without
 * the lean kernel, before the first solve, and for a plan created under SRH_LEAN_NO_TOEPLITZ=1.  Waits for the solve. */
int sgusto_plan_single_region_qps(sgusto_plan_t *plan, int32_t *count);
/* The row roster of the half-size lean kernel's tile factorisation that this plan's constants were built with (SRH_LEAN_ROSTER=<code>
 * overrides the default when the plan is created; see slean_roster_replay for the codes); 0 for every other kernel. */
int sgusto_plan_lean_roster(const sgusto_plan_t *plan, int32_t *code);
/* 1 if this plan's constants were built under SRH_IPM_LATE_STOP=1 and a lean kernel serves it: the lean interior points then test
 * convergence behind the predictor's Newton system only (the former order), not before it.  0 otherwise, any other value of the
 * variable included. */
int sgusto_plan_ipm_late_stop(const sgusto_plan_t *plan, int32_t *late);
int sgusto_plan_solve(sgusto_plan_t *plan, const double *x0, const double *u_init, const double *x_init,
                      const double *z, const double *zf, const double *u_des, double *xopt, double *uopt,
                      double *zopt, int32_t *iters, int32_t *status, double *trace);
int sgusto_plan_solve_dev(sgusto_plan_t *plan, const double *x0, const double *u_init, const double *x_init,
                          const double *z, const double *zf, const double *u_des, double *xopt, double *uopt,
                          double *zopt, int32_t *iters, int32_t *status, double *trace, void *stream);

/* Asynchronous form of sgusto_plan_solve -- the `send_request(wait=False)` / `check_if_done` / `force_wait` protocol
 * of the reference's solver client (scp/ros.py:183-223; used by tpwl/controllers.py:276-292,327): `_begin` copies
 * the host inputs into the plan's pinned staging block, enqueues H2D copies, the solve and the D2H copies of the
 * results on the plan's own (non-blocking) stream and returns; `_done` polls the completion event without blocking;
 * `_end` waits for it and hands the results over.  One request per plan at a time. */
int sgusto_plan_prepare_async(sgusto_plan_t *plan);   /* optional: create the stream / pinned block now (~10 ms) */
int sgusto_plan_solve_begin(sgusto_plan_t *plan, const double *x0, const double *u_init, const double *x_init,
                            const double *z, const double *zf, const double *u_des, int want_trace);
int sgusto_plan_solve_done(sgusto_plan_t *plan, int *done);
int sgusto_plan_solve_end(sgusto_plan_t *plan, double *xopt, double *uopt, double *zopt, int32_t *iters,
                          int32_t *status, double *trace);

/* The device-side duration (ms) of the last request collected by sgusto_plan_solve_end: from the first host-to-device copy
 * to the last device-to-host copy on the plan's stream (HIP events) -- the solver's own time, what the reference reports
 * as its solve time (scp/ros.py:116-124), independent of when the caller came back for the result; -1 before the first. */
int sgusto_plan_last_async_ms(sgusto_plan_t *plan, double *ms);

/* Batched closed loop on a resident TPWL GuSTO plan (csrc/gusto_loop.hip): every rollout b of the plan's batch is its own
 * receding-horizon loop -- plan, apply n_keep inputs to a TPWL plant discretised at dt_sim, shift, re-plan from the plant state
 * (the reference's `mpc=True` policy, tpwl/controllers.py:269-274, with perfect state feedback) -- and nothing but the run's
 * records crosses PCIe.  Period k (k counts from the last reset; t_k = t_start + k (n_keep dt_sim)):
 *   x0      = the plant state
 *   guess   k = 0: u_init = 0, x_init = the zero-input rollout of the PLANNER's model from x0 (scp/standalone.py:32-33);
 *           k > 0: the previous xopt / uopt from row idx0 on, their last row held over the rest (scp/ros.py:110-114), idx0 = the
 *           first j with t_{k-1} + dt j >= t_k
 *   target  z[b][j] = the installed table (t, z) interpolated linearly at (t_k + phase[b]) + dt j, j = 0..N, clamped to its first /
 *           last row outside the table (standalone.py:29); zf = z[b][N] when the plan has a terminal cost; u_des alike on rows 0..N-1
 *   solve   sgusto_plan_solve_dev; a rollout that ends with status 1 / 2 / 3 goes on with what the kernel returned
 *   advance for s = 0..n_keep-1, tau = s dt_sim, j = min((int)(tau / dt), N - 1), theta = (tau - j dt) / dt:
 *           x_bar = xopt[j] + theta (xopt[j+1] - xopt[j]); u_bar the same on [uopt ; uopt[N-1]] (controllers.py:299);
 *           u = u_bar + K[i] (x - x_bar), i = nearest point of the PLANNER's table at x_bar (controllers.py:330-331), or u = u_bar
 *           without gains;  x <- A_d[p] x + B_d[p] u + d_d[p] (+ w), p = nearest point of the PLANT's table at x;  z = H x, H the
 *           planner model's output map (as zopt = H xopt, gusto.py:486).
 * The schedule (t_k, idx0, j, theta) is the same for every rollout and is computed on the host in double precision
 * (sgusto_loop_schedule: host arithmetic only).  f64 throughout; n_x <= 128, n_u <= 16.  The plan and both models must outlive the
 * loop; the plan's iteration cap is the one in force when sgusto_loop_run is called.
 * create refuses n_keep dt_sim > N dt (the shift would find no row), a plant of other dimensions or without discrete tables, and a
 * planner model without an output map of the plan's n_z.  max_steps_per_run bounds periods * n_keep of one run (the pinned record
 * blocks are sized by it). */
typedef struct sgusto_loop sgusto_loop_t;
int sgusto_loop_create(sgusto_loop_t **out, sgusto_plan_t *plan, stpwl_t *planner_model, stpwl_t *plant, double dt_sim, int n_keep,
                       int64_t max_steps_per_run);
int sgusto_loop_destroy(sgusto_loop_t *h);
/* t (T, increasing), z (T x n_z), u_des (T x n_u) or NULL, phase (batch) or NULL = zeros */
int sgusto_loop_set_target(sgusto_loop_t *h, int T, const double *t, const double *z, const double *u_des, const double *phase);
int sgusto_loop_set_feedback(sgusto_loop_t *h, const double *K);          /* P x n_u x n_x of the planner's points; NULL: none */
int sgusto_loop_reset(sgusto_loop_t *h, const double *x0, double t_start);        /* x0 (batch x n_x) */
/* `periods` periods enqueued on the handle's own stream, the records copied back once, ONE blocking wait.  W (periods x n_keep x
 * batch x n_x) or NULL: added to the plant's next state, uploaded once.  With S = periods n_keep: X_cl (batch x (S + 1) x n_x) or
 * NULL, Z_cl (batch x (S + 1) x n_z), U_cl (batch x S x n_u), row 0 = the state the run started from; iters, status, J
 * (periods x batch).  A following run continues: time, plant states, previous plan. */
int sgusto_loop_run(sgusto_loop_t *h, int periods, const double *W, double *X_cl, double *Z_cl, double *U_cl, int32_t *iters,
                    int32_t *status, double *J);
/* The solver inputs / the plan of the last period (any may be NULL; zf, u_des are left alone when the loop has none). */
int sgusto_loop_last_inputs(sgusto_loop_t *h, double *x0, double *u_init, double *x_init, double *z, double *zf, double *u_des);
int sgusto_loop_last_plan(sgusto_loop_t *h, double *xopt, double *uopt);
/* The advance kernel alone -- the launch sgusto_loop_run makes -- on host-supplied plans: xopt (batch x (N+1) x n_x), uopt (batch x N
 * x n_u), x (batch x n_x), W (n_keep x batch x n_x) or NULL -> X (batch x n_keep x n_x), Z (batch x n_keep x n_z), U (batch x n_keep
 * x n_u), and the points picked at every sub-step, idx_plant / idx_gain (batch x n_keep; idx_gain = -1 without gains; either may be
 * NULL).  The loop's own state is not touched. */
int sgusto_loop_advance(sgusto_loop_t *h, const double *xopt, const double *uopt, const double *x, const double *W, double *X,
                        double *Z, double *U, int32_t *idx_plant, int32_t *idx_gain);
/* ---- the observed loop: output feedback through `batch` extended Kalman filters (sekf_batch_t) inside the loop, as the reference's
 * TemplateController.evaluate closes it (tpwl/controllers.py:85-117: observer.update(u_prev, y, dt) at every simulation step, plan and
 * control from observer.x).  Period k as above with three changes: the solver's x0 is the estimate x_hat; the law reads the estimate,
 * u = u_bar + K[i] (x_hat - x_bar); and after the plant step of sub-step s
 *           y = C x + y_ref (+ v_s);  (x_hat, Sigma) <- predictor with this u on the FILTER model's region nearest to x_hat, then the
 *           update with y  (C, y_ref and the filter's model are the observer's own; its model need not be the plant).
 * A filter whose innovation covariance is not positive definite keeps its estimate; the loop goes on and the status is recorded.
 * Launches of a period: prepare -> solve -> costs -> n_keep x (advance of one sub-step -> batched filter step -> record), all on the
 * handle's stream; still ONE host wait per run.
 * set_observer: the filters of the loop (NULL detaches them); refused unless batch, n_x and n_u are the loop's and the filter's model is
 * pre-discretised.  The observer must outlive the loop, and nothing else may step it while a run is in flight. */
int sgusto_loop_set_observer(sgusto_loop_t *h, sekf_batch_t *observer);
/* x0 (batch x n_x) plant states, x_hat0 (batch x n_x) estimates or NULL = x0: where the reference's first observer.update at t = 0
 * leaves the filters.  Every filter's covariance is re-installed from Sigma0. */
int sgusto_loop_reset_observed(sgusto_loop_t *h, const double *x0, const double *x_hat0, double t_start);
/* sgusto_loop_run with the filters in the loop.  V (periods x n_keep x batch x n_y) or NULL: measurement noise.  Xhat (batch x (S + 1)
 * x n_x): row 0 the estimates the run started from, row s + 1 the estimate after sub-step s; Y_cl (batch x S x n_y); ekf_status
 * (periods x batch): the OR of the period's filter statuses.  Needs sgusto_loop_reset_observed; sgusto_loop_run refuses to continue
 * such a state. */
int sgusto_loop_run_observed(sgusto_loop_t *h, int periods, const double *W, const double *V, double *X_cl, double *Z_cl, double *U_cl,
                             int32_t *iters, int32_t *status, double *J, double *Xhat, double *Y_cl, int32_t *ekf_status);
/* The observed sub-step chain of one period alone -- the launches sgusto_loop_run_observed makes -- on host-supplied plans, states x and
 * estimates x_hat (batch x n_x), W (n_keep x batch x n_x) / V (n_keep x batch x n_y) or NULL -> X, Z, U as sgusto_loop_advance, Xhat
 * (batch x n_keep x n_x) the estimate after every sub-step, Y (batch x n_keep x n_y), the three points picked at every sub-step
 * (plant at x, gain at x_bar, filter at x_hat; batch x n_keep, any may be NULL) and ekf_status (batch, or NULL).  The attached filters
 * are started from x_hat and Sigma0 and left where the chain ends: the loop needs a reset afterwards. */
int sgusto_loop_advance_observed(sgusto_loop_t *h, const double *xopt, const double *uopt, const double *x, const double *x_hat, const double *W,
                                 const double *V, double *X, double *Z, double *U, double *Xhat, double *Y, int32_t *idx_plant,
                                 int32_t *idx_gain, int32_t *idx_filter, int32_t *ekf_status);
/* periods run since the last reset, and the blocking host waits of the last run */
int sgusto_loop_stats(sgusto_loop_t *h, int64_t *steps, int64_t *waits_last_run);
/* The schedule of period k (no GPU): *t_k, *idx0 (0 for k = 0), j (n_keep), theta (n_keep).  Any output may be NULL. */
int sgusto_loop_schedule(int N, double dt, double dt_sim, int n_keep, double t_start, int64_t k, double *t_k, int *idx0, int32_t *j,
                         double *theta);
/* ---- the chained policy: the reference's `mpc=False` (tpwl/controllers.py:236, its default, and what its TPWL drivers run).  Period 0
 * after a reset is as above.  Period k >= 1 starts from the END of the part of plan k - 1 that the robot follows,
 *   x0      = xopt[j_end] + theta_end (xopt[j_end + 1] - xopt[j_end])  of the previous plan (controllers.py:272: x_opt[-1]),
 *             (j_end, theta_end) = the schedule's rule of a sub-step at tau = n_keep dt_sim (sgusto_loop_end_row),
 * not from the plant state or the estimate: the plans do not depend on the plant, only the law and the filters close the loop.  Guess,
 * target, solve and advance are unchanged; row 0 of the X / Z records is the plant's state as before.  One more launch per period,
 * behind the solve: loop_chain_kernel forms x0 of the next period and the period's rows of the nominal tape the reference stitches
 * (controllers.py:302-315; x_opt / u_opt of save_controller_info): Xbar (batch x (S + 1) x n_x), Ubar (batch x (S + 1) x n_u), row
 * p n_keep + s the plan of period p at tau = s dt_sim (s = n_keep: at tau_end; the input held over the plan's last interval).  At a
 * junction row k n_keep, k >= 1, Xbar keeps the OLD plan's end (x_opt_new[1:] is appended) and Ubar takes the NEW plan's first row
 * (u_opt[:-1] is kept); row 0 of a run that continues another is the old plan's end as well.
 * set_chained: on != 0 selects the policy, 0 the default (re-plan from the plant).  Refused unless no period has run since the
 * create or the last reset.  The chain state lives in the handle: runs continue it, a reset drops it. */
int sgusto_loop_set_chained(sgusto_loop_t *h, int on);
/* sgusto_loop_run (Xhat, Y_cl, ekf_status and V all NULL) or sgusto_loop_run_observed (all three records given) with the tape: Xbar,
 * Ubar as above, either may be NULL.  Asking for a tape is refused unless the loop is chained. */
int sgusto_loop_run_tape(sgusto_loop_t *h, int periods, const double *W, const double *V, double *X_cl, double *Z_cl, double *U_cl,
                         int32_t *iters, int32_t *status, double *J, double *Xhat, double *Y_cl, int32_t *ekf_status, double *Xbar, double *Ubar);
/* The end row of the schedule (no GPU): tau = n_keep dt_sim, *j_end = min((int)(tau / dt), N - 1), *theta_end = (tau - j_end dt) / dt.
 * At n_keep dt_sim == N dt: j_end = N - 1 and theta_end is 1 to rounding.  Either output may be NULL. */
int sgusto_loop_end_row(int N, double dt, double dt_sim, int n_keep, int32_t *j_end, double *theta_end);
/* The chain kernel alone -- the launch a chained period makes, in its period-0 form -- on host-supplied plans: xopt (batch x (N+1) x n_x),
 * uopt (batch x N x n_u) -> x_next (batch x n_x), Xbar_rows (batch x (n_keep + 1) x n_x), Ubar_rows (batch x (n_keep + 1) x n_u), rows
 * s = 0..n_keep; any output may be NULL.  The loop's own state is not touched. */
int sgusto_loop_chain(sgusto_loop_t *h, const double *xopt, const double *uopt, double *x_next, double *Xbar_rows, double *Ubar_rows);

/* Batched closed loop on a resident SSM GuSTO plan (csrc/gusto_ssm_loop.hip): the loop of the reference's hardware driver
 * (examples/hardware/diamond_SSM.py:353-361, SSM/controllers.py: the scp controller applies u = u_bar(t) with no feedback gain, the
 * SSMObserver is the polynomial map x_hat = W_map(y - z_ref)), one per rollout b of the plan's batch.  Period k as sgusto_loop's
 * (same schedule: sgusto_loop_schedule; same shift and target window: one prepare kernel for both units) with
 *   x0      = the estimate x_hat (observe = 1) or the plant state (observe = 0)
 *   guess   k = 0: u_init = 0, x_init = the zero-input rollout of the PLANNER's model at dt (sssm_rollout_dev in the plan's mode)
 *   target  z in the shifted coordinates of the plan (without z_ref); an SSM plan has no terminal cost, so there is no zf
 *   solve   sgusto_ssm_plan_solve_dev with trace = NULL; whatever status a rollout ends with, it goes on with what the kernel returned
 *   advance ONE launch for all n_keep sub-steps, s = 0..n_keep-1 with (j, theta) of the schedule:
 *           u      = [uopt ; uopt[N-1]] interpolated at (j, theta)                      (SSM/controllers.py:204, 237)
 *           x     <- A_d x + B_d u + d_d (+ w), (A_d, B_d, d_d) the PLANT's Jacobians at (x, u) discretised at dt_sim in plant_mode
 *                    (1 fe, 2 be, 3 bil, 4 its discrete map; ssm.py:198-218, 279-301)
 *           zeta   = C_plant(x)                  the record Z: without z_ref, like the plan's z
 *           y      = (zeta + z_ref_plant) + v    in this order of additions
 *           x_hat  = V_planner phi_s(y - z_ref_planner)                                 (SSMObserver.update with the controller's model)
 * f64 throughout.  The plant may be the planner's model or another one of the same n_x, n_u, n_o (= n_x); its tables, the planner's V
 * and z_ref and the work area live in LDS for the launch: what exceeds 160 KiB is refused at creation with the byte count.  create also
 * refuses a plan with rate rows (a rollout whose trust region binds comes back with status -78 for the host loop, which a device loop
 * cannot serve), a plant of other dimensions or without a discrete map when plant_mode = 4, n_u > 16, and n_keep dt_sim > N dt.
 * The plan and both models must outlive the loop; the plan's iteration cap is the one in force when sgusto_ssm_loop_run is called. */
typedef struct sgusto_ssm_loop sgusto_ssm_loop_t;
int sgusto_ssm_loop_create(sgusto_ssm_loop_t **out, sgusto_ssm_plan_t *plan, sssm_t *planner_model, sssm_t *plant, int plant_mode,
                           double dt_sim, int n_keep, int observe, int64_t max_steps_per_run);
int sgusto_ssm_loop_destroy(sgusto_ssm_loop_t *h);
/* t (T, increasing), z (T x n_z), u_des (T x n_u) or NULL, phase (batch) or NULL = zeros */
int sgusto_ssm_loop_set_target(sgusto_ssm_loop_t *h, int T, const double *t, const double *z, const double *u_des, const double *phase);
/* x0 (batch x n_x) plant states, v0 (batch x n_o) or NULL: the noise of the first measurement.  The advance kernel, launched with zero
 * sub-steps, forms zeta0 = C_plant(x0), y0 = (zeta0 + z_ref_plant) + v0 and x_hat0 = W_map(y0 - z_ref_planner): the reference's first
 * observer.update before its first compute_policy.  Waits for the launch. */
int sgusto_ssm_loop_reset(sgusto_ssm_loop_t *h, const double *x0, const double *v0, double t_start);
/* `periods` periods (prepare -> solve -> costs -> advance each) enqueued on the handle's own stream, the records copied back once, ONE
 * blocking wait.  W (periods x n_keep x batch x n_x), V (periods x n_keep x batch x n_o) or NULL.  With S = periods n_keep: X_cl
 * (batch x (S + 1) x n_x) or NULL, Z_cl, Y_cl (batch x (S + 1) x n_o), Xhat (batch x (S + 1) x n_x), U_cl (batch x S x n_u); row 0 =
 * where the run started (after a reset: x0, zeta0, y0, x_hat0); iters, status, J (periods x batch).  A following run continues. */
int sgusto_ssm_loop_run(sgusto_ssm_loop_t *h, int periods, const double *W, const double *V, double *X_cl, double *Z_cl, double *U_cl,
                        double *Y_cl, double *Xhat, int32_t *iters, int32_t *status, double *J);
/* The solver inputs / the plan of the last period (any may be NULL; z, u_des are left alone when the loop has none). */
int sgusto_ssm_loop_last_inputs(sgusto_ssm_loop_t *h, double *x0, double *u_init, double *x_init, double *z, double *u_des);
int sgusto_ssm_loop_last_plan(sgusto_ssm_loop_t *h, double *xopt, double *uopt);
/* periods run since the last reset, and the blocking host waits of the last run */
int sgusto_ssm_loop_stats(sgusto_ssm_loop_t *h, int64_t *steps, int64_t *waits_last_run);
/* The advance kernel alone -- the launch sgusto_ssm_loop_run makes -- on host arrays, through temporary buffers, without a plan or a
 * loop handle: j, theta (n_keep) of the schedule, uopt (batch x N x n_u), x (batch x n_x), W (n_keep x batch x n_x) / V (n_keep x
 * batch x n_o) or NULL -> X, Xhat (batch x n_keep x n_x), Z, Y (batch x n_keep x n_o), U (batch x n_keep x n_u) after every sub-step.
 * xopt (batch x (N+1) x n_x) is accepted for symmetry with sgusto_loop_advance and not read: the law has no gain.  observer_model:
 * the model whose V and z_ref form x_hat (it may be the plant). */
int sgusto_ssm_loop_advance(sssm_t *plant, int plant_mode, sssm_t *observer_model, double dt_sim, int N, int n_keep, int64_t batch,
                            const int32_t *j, const double *theta, const double *xopt, const double *uopt, const double *x,
                            const double *W, const double *V, double *X, double *Z, double *U, double *Y, double *Xhat);
/* The same loop on a nearest-point TPWL plant of n_p states (the reference's drivers: the controller sees only the measured tip).  The
 * handle is an sgusto_ssm_loop with a plant kind: reset, run, set_target, last_inputs, last_plan, stats and destroy serve both kinds;
 * with a TPWL plant x0, W and the X record have n_p columns, and the plans always start from the estimate.  C (n_o x n_p), y_ref (n_o):
 * the measurement of the plant state.  Sub-step s of the ONE advance launch of a period (ssm_loop_advance_tpwl_kernel):
 *           u      = [uopt ; uopt[N-1]] interpolated at (j, theta), no gain
 *           i      = the plant's nearest point to x (the point-search rule of csrc/tpwl_dev.h; a state that is not a number picks 0)
 *           x     <- d_d[i] + A_d[i] x + B_d[i] u (the step rule of csrc/tpwl_dev.h) (+ w)
 *           zeta   = C x                         the record Z: without y_ref
 *           y      = (zeta + y_ref) + v          in this order of additions
 *           x_hat  = V_planner phi_s(y - z_ref_planner)
 * Refused by name, with the numbers, before any launch: n_p > 128, n_u > 16, n_o other than the planner model's, a planner model whose
 * n_x, n_u are not the plan's, a plant whose n_u is not the plan's, a plant without discrete tables (it must be pre-discretised at
 * dt_sim), an LDS request above 160 KiB, a plan with rate rows, n_keep dt_sim > N dt. */
int sgusto_ssm_loop_create_tpwl(sgusto_ssm_loop_t **out, sgusto_ssm_plan_t *plan, sssm_t *planner_model, stpwl_t *plant, const double *C,
                                const double *y_ref, int n_o, double dt_sim, int n_keep, int64_t max_steps_per_run);
/* The TPWL-plant advance kernel alone on host arrays, as sgusto_ssm_loop_advance: x (batch x n_p), W (n_keep x batch x n_p), V (n_keep x
 * batch x n_o) or NULL -> X (batch x n_keep x n_p), Z, Y (batch x n_keep x n_o), U (batch x n_keep x n_u), Xhat (batch x n_keep x n_x of
 * the observer model), idx (batch x n_keep) the plant's point of every sub-step. */
int sgusto_ssm_loop_advance_tpwl(stpwl_t *plant, const double *C, const double *y_ref, int n_o, sssm_t *observer_model, double dt_sim, int N,
                                 int n_keep, int64_t batch, const int32_t *j, const double *theta, const double *uopt, const double *x,
                                 const double *W, const double *V, double *X, double *Z, double *U, double *Y, double *Xhat, int32_t *idx);
/* The admissible set of the measurements for either plant kind (SSM/controllers.py:96-97): Y = {y : A y <= b}, A (rows x n_o) row-major.
 * From the next reset on every measurement y -- the reset's first one included -- that lies outside Y is replaced by its Euclidean
 * projection inside the advance kernel, and the estimate reads y_used - z_ref_planner (the device function of spoly_project: the same
 * bits; a sample without a projection is used as it is and reported by its status word, spoly_project_status).  n_o <= 16, rows <= 64,
 * A and b finite, and a loop created with observe = 0 are refused with the numbers.  A = NULL or b = NULL removes Y.  The loop needs a
 * reset behind either. */
int sgusto_ssm_loop_set_reproject(sgusto_ssm_loop_t *h, const double *A, const double *b, int rows);
/* sgusto_ssm_loop_run with the two records of the re-projection: Y_used (batch x (S + 1) x n_o) the measurements as the observer map read
 * them, proj (batch x (S + 1)) their status words; row 0 = where the run started.  Y_cl stays the raw measurement. */
int sgusto_ssm_loop_run_reprojected(sgusto_ssm_loop_t *h, int periods, const double *W, const double *V, double *X_cl, double *Z_cl,
                                    double *U_cl, double *Y_cl, double *Xhat, int32_t *iters, int32_t *status, double *J, double *Y_used,
                                    int32_t *proj);
/* The two advance kernels alone with a Y (YA (y_rows x n_o), Yb): as sgusto_ssm_loop_advance / _advance_tpwl, and Y_used (batch x n_keep x
 * n_o), proj (batch x n_keep) of every sub-step. */
int sgusto_ssm_loop_advance_reprojected(sssm_t *plant, int plant_mode, sssm_t *observer_model, double dt_sim, int N, int n_keep, int64_t batch,
                                        const int32_t *j, const double *theta, const double *uopt, const double *x, const double *W,
                                        const double *V, const double *YA, const double *Yb, int y_rows, double *X, double *Z, double *U,
                                        double *Y, double *Xhat, double *Y_used, int32_t *proj);
int sgusto_ssm_loop_advance_tpwl_reprojected(stpwl_t *plant, const double *C, const double *y_ref, int n_o, sssm_t *observer_model,
                                             double dt_sim, int N, int n_keep, int64_t batch, const int32_t *j, const double *theta,
                                             const double *uopt, const double *x, const double *W, const double *V, const double *YA,
                                             const double *Yb, int y_rows, double *X, double *Z, double *U, double *Y, double *Xhat,
                                             int32_t *idx, double *Y_used, int32_t *proj);

/* =====================================================================================================
 * Koopman baseline. reference: sofacontrol/baselines/koopman/koopman_utils.py, koopman/koopman.py, baselines/ros.py:139-235
 * zeta = [y_t, y_{t-1} .. y_{t-d}, u_{t-1} .. u_{t-d}] of scaled samples (KoopmanData.get_zeta, koopman_utils.py:30-47;
 * scale_down = (v - offset) / factor, 104-107), nzeta = n_y (d + 1) + m d; psi = the monomials of zeta of degree 1 .. degree
 * in the order of get_lifting_function (koopman_utils.py:156-175: sympy grlex over the REVERSED variables), then the constant
 * (dmd = 0) or no constant (dmd = 1); the lift writes W psi when W (n_w x n_psi) is given and is not the identity, else psi.
 * Limits: nzeta <= 64, degree <= 4, n_psi <= 1024 (beyond them skoop_create fails with SRH_EINVAL).
 * ===================================================================================================== */
typedef struct skoop skoop_t;
int skoop_num_observables(int nzeta, int degree, int dmd);                 /* n_psi (0 on bad arguments) */
int skoop_exponents(int nzeta, int degree, int dmd, int32_t *exps);        /* (n_psi x nzeta), the constant row last unless dmd */
/* KoopmanModel + KoopmanScaling: y_offset / y_factor (n_y), u_offset / u_factor (m); W (n_w x n_psi) or NULL; batch = the
 * problems of the online ring (skoop_push) and of an MPC plan on this handle. */
int skoop_create(skoop_t **out, int n_y, int m, int delays, int degree, int dmd, const double *y_offset, const double *y_factor,
                 const double *u_offset, const double *u_factor, const double *W, int n_w, int64_t batch);
int skoop_destroy(skoop_t *h);
int skoop_info(skoop_t *h, int *nzeta, int *n_psi, int *n_out, int *has_w);   /* n_out = columns the lift writes */
/* lift_data for rows of zeta (rows x nzeta) -> (rows x n_out) */
int skoop_lift(skoop_t *h, const double *zeta, int64_t rows, double *out);
int skoop_lift_dev(skoop_t *h, const double *zeta_dev, int64_t rows, double *out_dev, void *stream);
/* add_zeta_offline (koopman_utils.py:75-83) + lift over a raw record y (T x n_y), u (T x m) (unscaled): row i - d for
 * i = d .. T-1, so (T - d) x n_out rows; nothing when T < d + 1. */
int skoop_embed_lift(skoop_t *h, const double *y, const double *u, int64_t T, double *out);
int skoop_embed_lift_dev(skoop_t *h, const double *y_dev, const double *u_dev, int64_t T, double *out_dev, void *stream);
/* Online ring (KoopmanData.add_measurement, 16-28): the last d + 1 scaled samples of every problem of the batch.  skoop_push
 * takes y (batch x n_y), u (batch x m) through the handle's pinned block and is asynchronous on the handle's stream;
 * skoop_ring_lift_dev writes the lift of the current zeta of every problem to out_dev (batch x n_out) on that stream. */
int skoop_push(skoop_t *h, const double *y, const double *u);
int skoop_reset(skoop_t *h);
int skoop_state_dev(skoop_t *h, const double **ring_dev, int *slots, int *head, int64_t *count, void **stream);
int skoop_ring_lift_dev(skoop_t *h, double *out_dev);
/* Resident Koopman MPC (MPCSolverNode.mpc_callback, baselines/ros.py:202-235): an slocp plan of `batch` problems with
 * A (n_x x n_x), B (n_x x n_u) tiled over the horizon once in HBM (d_d = 0) and prob->tr_active = 0, n_x = n_out.
 * skoop_mpc_step: [push y, u_prev (both NULL: none)] -> lift the ring into the plan's x0 -> slocp_plan_solve_dev -> one copy
 * of (x0, x, u, J, status) back, one synchronisation.  z (batch x (N+1) x n_z), zf (batch x n_z), u_des (batch x N x n_u):
 * NULL keeps the last given (none given: no target).  x0 (batch x n_x) may be NULL. */
typedef struct skoop_mpc skoop_mpc_t;
int skoop_mpc_create(skoop_mpc_t **out, skoop_t *h, const slocp_problem *prob, const double *A, const double *B);
int skoop_mpc_destroy(skoop_mpc_t *plan);
int skoop_mpc_step(skoop_mpc_t *plan, const double *y, const double *u_prev, const double *z, const double *zf,
                   const double *u_des, double *x0, double *x, double *u, double *J, int32_t *status);
/* Step records for probes and tests.  skoop_mpc_set_timing(plan, 1) brackets the parts of every following step with HIP events on
 * the handle's stream; skoop_mpc_stats then gives the steps taken, the blocking host waits the last step made (event or stream
 * synchronisations, counted where they are made) and ms[4] of the last step: [step start .. QP launch] (push, targets, lift),
 * [QP] (slocp_plan_solve_dev_resident: its transposes when the horizon is new, then the QP kernels), [results copied back],
 * [whole step on the device]; -1 while timing is off. */
int skoop_mpc_set_timing(skoop_mpc_t *plan, int on);
int skoop_mpc_stats(skoop_mpc_t *plan, int64_t *steps, int64_t *waits_last_step, double *ms);

/* Koopman model identification (EDMD, csrc/koopman_fit.hip): records (y, u) -> a model (A, B) for the lift of an skoop_t handle.
 * THE FIT (this text defines it; the reference's model came from an external MATLAB trainer that is not part of it):
 *   records   E episodes, each y (T x n_y), u (T x m), raw; `stride` s >= 1 keeps rows 0, s, 2s, .. of every episode (a record at
 *             dt_sim read at Ts = s dt_sim; row i s carries the input held over the step); T' = the rows kept.
 *   zeta_i    [y_i, y_{i-1} .. y_{i-d}, u_{i-1} .. u_{i-d}] of scaled samples for kept row i >= d: what skoop_embed_lift builds;
 *             psi_i = psi(zeta_i), the handle's observables (the constant last unless dmd).
 *             A scaled sample is (v - offset) / factor rounded once: within one ulp of the lift's own, which rounds the subtraction
 *             and the division separately (a term of G is a product of up to 2 degree samples and inherits each one's error).
 *   v_i       scale_down(u[i + u_lag]); u_lag = 0: row i holds the input applied AFTER y_i (the closed loops' results), u_lag = 1:
 *             the input applied BEFORE y_i (the rows KoopmanData.add_measurement and the device ring keep).
 *   pairs     (i, i + 1) for d <= i <= T' - 2, never across an episode; an episode with T' <= d + 1 contributes nothing.
 *   sums      Phi_i = [psi_i; v_i] (n = n_psi + m): G = sum Phi_i Phi_i^T (n x n), R = sum psi_{i+1} Phi_i^T (n_psi x n),
 *             Q = sum |psi_{i+1}|^2, S = the number of pairs.
 *   model     [A B] = R (G + ridge I)^-1, ridge >= 0: the minimiser of sum |psi_{i+1} - A psi_i - B v_i|^2 + ridge |[A B]|_F^2.
 *   scaling   the handle's, or computed from the records over the kept rows: offset = (max + min) / 2, factor = (max - min) / 2
 *             (skoop_fit_minmax; a channel with max == min is refused by name).
 * Not offered: the trainer's L1 (lasso) constraint, sample weights, non-polynomial observables, truncation (a handle with W is
 * refused).  Limits (SRH_EINVAL before any device call): n = n_psi + m <= 128 and the lift's own.  The sums are accumulated on f64
 * MFMA without floating-point atomics, in an order fixed by (E, T, stride, d) and the model's shape: the same records give the same
 * bits.  All calls on one handle are ordered by the caller (one stream, or synchronised between streams).
 * skoop_fit_plan answers on the host (no GPU): n_psi, n, the pairs of a chunk of the accumulate kernel and its dynamic LDS; any
 * output may be NULL; SRH_EINVAL when the shape is refused. */
typedef struct skoop_fit skoop_fit_t;
int skoop_fit_plan(int nzeta, int degree, int dmd, int m, int *n_psi, int *n, int *rows_per_chunk, int64_t *lds_bytes);
int skoop_fit_create(skoop_fit_t **out, skoop_t *lift);     /* the lift handle must outlive the fit handle */
int skoop_fit_destroy(skoop_fit_t *f);
int skoop_fit_reset(skoop_fit_t *f);                        /* sums and pairs back to zero */
/* records -> the four scale vectors (n_y, n_y, m, m); the reduction runs on the device in a fixed order; the _dev form takes
 * device records and synchronises `stream` before it returns */
int skoop_fit_minmax(const double *y, const double *u, int64_t E, int64_t T, int n_y, int m, int stride, double *y_offset,
                     double *y_factor, double *u_offset, double *u_factor);
int skoop_fit_minmax_dev(const double *y_dev, const double *u_dev, int64_t E, int64_t T, int n_y, int m, int stride, double *y_offset,
                         double *y_factor, double *u_offset, double *u_factor, void *stream);
/* y (E x T x n_y), u (E x T x m) are added to the handle's sums; may be called many times.  The _dev form is asynchronous on
 * `stream`. */
int skoop_fit_add(skoop_fit_t *f, const double *y, const double *u, int64_t E, int64_t T, int stride, int u_lag);
int skoop_fit_add_dev(skoop_fit_t *f, const double *y_dev, const double *u_dev, int64_t E, int64_t T, int stride, int u_lag, void *stream);
/* G (n x n), R (n_psi x n), Q (1), pairs (1); any may be NULL */
int skoop_fit_sums(skoop_fit_t *f, double *G, double *R, double *Q, int64_t *pairs);
/* A (n_psi x n_psi), B (n_psi x m).  info (optional): -1, or the failing pivot of G + ridge I -- not positive, not finite (a NaN of the
 * records ends here), or not above n eps of its diagonal entry, where its sign would be rounding noise -- (SRH_ENUMERIC, "increase
 * ridge"), or n when the solution holds a non-finite entry that no pivot caught (SRH_ENUMERIC); A and B are written on success only.
 * SRH_EINVAL when no pair has been added. */
int skoop_fit_solve(skoop_fit_t *f, double ridge, double *A, double *B, int32_t *info);

/* SSM model identification (csrc/ssm_fit.hip): records (y, u) -> rd_coeff / Bd, r_coeff / B, w_coeff of an SSM model (sssm_create).
 * THE FIT ("SSM model identification", defines it; the reference ships one trained model and no trainer):
 *   records   E episodes, each y (T x n_y), u (T x m), raw; `stride` s >= 1 keeps rows 0, s, 2s, .. of every episode; T' = the rows
 *             kept; row i holds the input applied after y_i.
 *   chart     x_i = V^T (y_i - y_ref), V (n_y x n_x) given; x is the exact sum rounded once (a compensated dot product).
 *             sssm_fit_cov returns C = sum (y - y_ref)(y - y_ref)^T over the kept rows, the matrix a PCA chart is read from.
 *   samples   the interior rows 1 <= i <= T' - 2 of every episode, never across an episode; T' < 3 contributes nothing.
 *   regressor Phi_i = [phi(x_i); u_i], phi = the monomials of sssm_exponents(n_x, P), P = max(rom_order, ssm_order); n = n_mon + m.
 *   sums      G = sum Phi_i Phi_i^T (n x n), R_d = sum x_{i+1} Phi_i^T (n_x x n), R_c = sum ((x_{i+1} - x_{i-1}) / (2 Ts)) Phi_i^T
 *             (n_x x n), R_w = sum (y_i - y_ref) phi(x_i)^T (n_y x n_mon), Q = the squared norms of the three targets, S = samples.
 *   solves    [rd_coeff Bd] from R_d and [r_coeff B] from R_c on the columns {monomials up to rom_order} + {inputs}; w_coeff from R_w
 *             on the monomials up to ssm_order.  Every block is equilibrated by its own diagonal: with D = diag(G_S),
 *             (D^-1/2 G_S D^-1/2 + ridge I) z = D^-1/2 r, coeff = D^-1/2 z, ridge >= 0 (relative to the unit diagonal).
 * Not offered: delay-embedded observations, a polynomial chart, separate autonomous and forced records, sample weights.
 * Limits (SRH_EINVAL before any device call): n <= 128, n_x <= 32, n_x <= n_y <= 64, orders <= 7, and the panel must fit the LDS.
 * The sums are accumulated on f64 MFMA without floating-point atomics: a workgroup sums a granule, eight consecutive 64-sample chunks
 * of one episode, and the granules join the running sums in order.  The same records give the same bits, and records split over
 * several add calls at episode boundaries give the bits of one call.  All calls on one handle are ordered by the caller.
 * sssm_fit_plan answers on the host (no GPU): n_mon, n, the samples of a chunk and the accumulate kernel's dynamic LDS; any output
 * may be NULL. */
typedef struct sssm_fit sssm_fit_t;
int sssm_fit_plan(int n_x, int n_y, int m, int rom_order, int ssm_order, int *n_mon, int *n, int *rows_per_chunk, int64_t *lds_bytes);
/* V (n_y x n_x); y_ref (n_y) or NULL for zeros */
int sssm_fit_create(sssm_fit_t **out, int n_x, int n_y, int m, int rom_order, int ssm_order, double Ts, const double *V, const double *y_ref);
int sssm_fit_destroy(sssm_fit_t *f);
int sssm_fit_reset(sssm_fit_t *f);                          /* sums and samples back to zero */
/* C (n_y x n_y) = sum over the kept rows of (y - y_ref)(y - y_ref)^T, count = the rows; reduced on the device in a fixed order.  The
 * _dev form takes device records and synchronises `stream` before it returns.  y_ref may be NULL (zeros). */
int sssm_fit_cov(const double *y, int64_t E, int64_t T, int n_y, int stride, const double *y_ref, double *C, int64_t *count);
int sssm_fit_cov_dev(const double *y_dev, int64_t E, int64_t T, int n_y, int stride, const double *y_ref, double *C, int64_t *count,
                     void *stream);
/* y (E x T x n_y), u (E x T x m) are added to the handle's sums; may be called many times.  The _dev form is asynchronous on `stream`. */
int sssm_fit_add(sssm_fit_t *f, const double *y, const double *u, int64_t E, int64_t T, int stride);
int sssm_fit_add_dev(sssm_fit_t *f, const double *y_dev, const double *u_dev, int64_t E, int64_t T, int stride, void *stream);
/* G (n x n), Rd (n_x x n), Rc (n_x x n), Rw (n_y x n_mon), Q (3: of x_{i+1}, the central difference, y_i - y_ref), samples; any may be NULL */
int sssm_fit_sums(sssm_fit_t *f, double *G, double *Rd, double *Rc, double *Rw, double *Q, int64_t *samples);
/* rd_coeff, r_coeff (n_x x nmon(n_x, rom_order)), Bd, B (n_x x m), w_coeff (n_y x nmon(n_x, ssm_order)).  info (2, optional): {-1, -1}, or
 * {the failing pivot's position in its block, its column of Phi} -- a pivot that is not positive, not finite, or not above n eps of
 * its (unit) diagonal entry (SRH_ENUMERIC; the message names the monomial or the input: "increase ridge"); {block size, -1} when a
 * solution holds a non-finite entry that no pivot caught.  SRH_EINVAL when no sample has been added. */
int sssm_fit_solve(sssm_fit_t *f, double ridge, double *rd_coeff, double *Bd, double *r_coeff, double *B, double *w_coeff, int32_t *info);

/* TPWL model identification (csrc/tpwl_fit.hip): records (x, u) of the reduced state and P linearisation points -> the tables A_c, B_c,
 * d_c, u of a TPWL model (stpwl_create).
 * THE FIT ("TPWL model identification", defines it; the reference builds its tables from the simulator's Jacobians):
 *   records   E episodes, each x (T x n_x), x = [v; q], n_x = 2 r, and u (T x m); row i holds the input applied after x_i; `stride`
 *             s >= 1 keeps rows 0, s, 2s, .. of every episode; T' = the rows kept.
 *   samples   the kept rows i <= T' - 2 of every episode (those with a kept successor), never across an episode; T' < 2 gives none.
 *   points    q, v (P x r) and the weights (w_q, w_v); x_p = [v_p; q_p].  p(i) = the nearest point to x_i by the point-search rule of
 *             stpwl_nearest (first minimum of w_q |q_p - q| + w_v |v_p - v|).
 *   regressor phi_i = [x_i - x_p; u_i; 1], n = n_x + m + 1; target g_i = (x_{i+1} - x_i) / Ts (the forward difference over kept rows:
 *             the fitted model is the one whose forward-Euler discretisation at Ts reproduces the one-step map).
 *   sums      per point over its samples: G_p = sum phi phi^T (n x n), R_p = sum g phi^T (n_x x n), Q_p = sum |g|^2, S_p = the samples.
 *   solve     per point, equilibrated by D = diag(G_p): (D^-1/2 G_p D^-1/2 + ridge I) z = D^-1/2 r, [A_c | B_c | c] = the rows D^-1/2 z,
 *             ridge >= 0 (relative to the unit diagonal); d_c = c - A_c x_p, so that xdot = A_c x + B_c u + d_c; u = the mean input of
 *             the point's samples.
 *   status    per point: 0 solved; 1 S_p < min_samples (a duplicated point: the first-minimum rule gives the later one no samples);
 *             2 a pivot that is not positive, not finite or not above n eps (1 + ridge), `column` = its column of phi (0 .. n_x - 1 a
 *             state, n_x .. n_x + m - 1 an input, n - 1 the constant), or n when the solution holds a non-finite entry that no pivot
 *             caught.  The tables of a point that did not solve are zeros.
 * Not offered: weighting-mode fits, sample weights, full-order records (project them first).  The points are the caller's;
 * stpwl_select_points (below) chooses them from the records by the reference's distance rule.
 * Limits (SRH_EINVAL before any device call): n <= 128, m <= 16 (stpwl_create's), P <= 1024, fewer than 2^31 kept rows per add call.
 * A kept row that is not finite (x or u) is refused by stpwl_fit_add / _add_dev with the episode and row of the first one; the sums
 * are untouched then.  The sums are accumulated on f64 MFMA without floating-point atomics: the kept rows are ordered by region with a
 * stable counting sort, a workgroup sums a granule (eight 64-entry chunks of one region's list), and the granules join the running
 * sums of their point in order.  The same sequence of add calls gives the same bits, and device records give the bits of host arrays;
 * two add calls do not give the bits of one (their ordered lists differ).  All calls on one handle are ordered by the caller.
 * stpwl_fit_plan answers on the host (no GPU): n, the entries of a chunk, the tiles a wave keeps in registers and the accumulate
 * kernel's dynamic LDS; any output may be NULL. */
typedef struct stpwl_fit stpwl_fit_t;
int stpwl_fit_plan(int P, int r, int m, int *n, int *rows_per_chunk, int *tiles_per_wave, int64_t *lds_bytes);
/* q, v (P x r) */
int stpwl_fit_create(stpwl_fit_t **out, int P, int r, int m, const double *q, const double *v, double w_q, double w_v, double Ts);
int stpwl_fit_destroy(stpwl_fit_t *f);
int stpwl_fit_reset(stpwl_fit_t *f);                        /* sums and counts back to zero */
/* x (E x T x n_x), u (E x T x m) are added to the handle's sums; may be called many times.  The _dev form reads device records on
 * `stream` and synchronises it before it returns. */
int stpwl_fit_add(stpwl_fit_t *f, const double *x, const double *u, int64_t E, int64_t T, int stride);
int stpwl_fit_add_dev(stpwl_fit_t *f, const double *x_dev, const double *u_dev, int64_t E, int64_t T, int stride, void *stream);
int stpwl_fit_counts(stpwl_fit_t *f, int64_t *counts);      /* (P) the samples of every point */
/* one point's G (n x n), R (n_x x n), Q (1), samples (1); any may be NULL */
int stpwl_fit_sums(stpwl_fit_t *f, int p, double *G, double *R, double *Q, int64_t *samples);
/* A_c (P x n_x x n_x), B_c (P x n_x x m), d_c (P x n_x), u (P x m), status (P), column (P).  min_samples < 0: the default n + 1.
 * SRH_EINVAL when no sample has been added; a point that does not solve is reported in status, not by the return code. */
int stpwl_fit_solve(stpwl_fit_t *f, double ridge, int64_t min_samples, double *A_c, double *B_c, double *d_c, double *u, int32_t *status,
                    int32_t *column);

/* TPWL point selection from records (csrc/tpwl_select.hip): the reference's distance rule (tpwl_utils.py:156-196) as a greedy scan over
 * recorded reduced states; what it returns goes into stpwl_fit_create unchanged.
 * THE SELECTION RULE ("TPWL model identification", defines it):
 *   records    x (E x T x n_x), x = [v; q], n_x = 2 r, and `stride` s >= 1 as for stpwl_fit_add.  The candidates are ALL kept rows
 *              0, s, 2s, .. of every episode (the last kept row too), scanned episode by episode and inside an episode in row order.
 *   points     the table starts as the seed q0, v0 (P0 x r each, P0 >= 0; NULL when P0 = 0).  With an empty table the first candidate is
 *              taken unconditionally (tpwl_utils.py:161-162).
 *   distances  of a candidate c to a point p: dq = w_q ||q_p - q_c||, dv = w_v ||v_p - v_c||, in the arithmetic of the point-search rule
 *              of stpwl_nearest: each squared norm summed by fma in the order j = 0, 1, ... from 0.0, then a correctly rounded sqrt.
 *              With w_v == 0 the velocity part is not read and dv = 0.
 *   decision   separate == 0 (tpwl_utils.py:193): c is taken iff dq + dv >= threshold for EVERY point of the table; separate != 0
 *              (tpwl_utils.py:187-191): iff dq >= threshold for every point, or dv >= threshold for every point.  A taken candidate
 *              joins the table before the next candidate is examined.
 *   cap        max_points counts the seed plus the taken points, max(P0, 1) <= max_points <= 1024 (the fit's limit on P).  When a
 *              candidate would become point max_points + 1 the scan stops there: status 1, stopped_at = that candidate; the rows behind
 *              it were not examined.
 * Outputs: count = the points of the table at the end (seed included); for the count - P0 taken points, in the order taken: index
 * ((max_points - P0) x 2 int64: episode, row in the UNstrided record), q and v ((max_points - P0) x r: bit-for-bit copies of the record's
 * entries), dmin ((max_points - P0), or x 2 when separate: min dq, min dv) = the smallest distance to the table at the moment the point
 * was taken, +inf for an unconditional first point; status 0 complete / 1 cap reached; stopped_at (2: episode, row; -1, -1 when
 * complete).  Any output other than count may be NULL.
 * Refused with SRH_EINVAL before anything is written: threshold not finite or <= 0; a weight negative or not finite, or both zero;
 * r < 1 (r <= 128); a seed entry that is not finite; a kept row that is not finite (the message names the episode and row of the first
 * one, as stpwl_fit_add does).
 * The answer does not depend on how the device splits the work (min is exact; no floating-point atomics), and scanning x1 and then x2
 * with the first result as the seed gives exactly the result of scanning their concatenation.  stpwl_select_points takes host records;
 * the _dev form reads device records in place on `stream` and synchronises it once, at the end.  stpwl_select_plan answers on the host
 * (no GPU): the candidates of a chunk, the dynamic LDS of the distance kernel and the launches of a call of `candidates` kept rows. */
int stpwl_select_plan(int r, int64_t candidates, int *chunk, int64_t *lds_bytes, int64_t *launches);
int stpwl_select_points(const double *x, int64_t E, int64_t T, int r, int stride, double w_q, double w_v, double threshold, int separate,
                        int P0, const double *q0, const double *v0, int max_points, int *count, int64_t *index, double *q, double *v,
                        double *dmin, int *status, int64_t *stopped_at);
int stpwl_select_points_dev(const double *x_dev, int64_t E, int64_t T, int r, int stride, double w_q, double w_v, double threshold,
                            int separate, int P0, const double *q0, const double *v0, int max_points, int *count, int64_t *index,
                            double *q, double *v, double *dmin, int *status, int64_t *stopped_at, void *stream);

/* TPWL horizon error (csrc/tpwl_horizon.hip): the k-step open-loop prediction error of a nearest-point TPWL model over records, read in
 * place on the device -- the reference's model check (examples/hardware/diamond.py:20-73 TPWL_rollout) for every window start at once.
 * THE HORIZON ERROR ("TPWL horizon error", defines it):
 *   records     x (E x T x n_x), u (E x T x m) and `stride` s >= 1 as for stpwl_fit_add (row i holds the input applied after x_i);
 *               T' = the rows kept.
 *   model       the handle's discrete tables (stpwl_create with A_d, B_d, d_d, or stpwl_set_discrete) and its output model, if set.
 *   windows     starts at the kept rows j0 = 0, w, 2w, .. (`every` = w >= 1) of every episode while j0 + H <= T' - 1, H = `horizon`;
 *               numbered episode by episode in row order; an episode with T' <= H has none; W = 0 windows is refused.
 *   prediction  xh_0 = x_{j0}; xh_{k+1} = A_d[i] xh_k + B_d[i] u_{j0+k} + d_d[i], i the nearest point to xh_k, k = 0 .. H - 1, in the
 *               arithmetic of stpwl_rollout: exactly its X for (x_{j0}, U[j0 : j0 + H]), bit for bit.
 *   errors      e_k = xh_k - x_{j0+k}; with an output model ez_k = H e_k (z_ref cancels).
 *   status      of a window: 0 ok; 1 some xh_k is not finite; 2 some record row the window reads (the states j0 .. j0 + H, the inputs
 *               j0 .. j0 + H - 1) is not finite; 2 wins over 1.  Only status-0 windows enter the sums and the maxima.
 * Outputs (any but counts may be NULL): sse (2 x (H + 1)): sse_x[k] = sum_w |e_k|^2, then sse_z[k] (zeros without an output model);
 * worst (2 x (H + 1)): max_w |e_k|_2, then of ez (-1 when no window has status 0); worst_at (2 x (H + 1) x 2 int64): episode and row in
 * the UNstrided record of the start of the window that attains it, ties to the lowest window number (-1, -1: none); counts (3 int64):
 * windows W, status-1 windows, status-2 windows; final_norms (2 x W): |e_H|_2, then |ez_H|_2 per window, NaN where status != 0; status
 * (W); x_pred (W x (H + 1) x n_x): the predictions, refused above the byte cap that stpwl_horizon_plan states (rows behind the one
 * at which a window left its loop are NaN).  Row k = 0 of every curve is exactly 0.
 * Bits: no floating-point atomics; the windows are dealt to workgroups in fixed blocks by window number (`block` windows of one episode)
 * and the blocks' partial sums are joined in block order, so the result is a function of the records and parameters alone: not of
 * the CU count, a rerun gives the same bits, and device records give the bits of host arrays.  max is exact.
 * Limits (SRH_EINVAL before any device call, with the offending number): n_x <= 128, m <= 16, 1 <= H <= 1024, stride, every >= 1; a
 * handle without discrete tables is refused.  stpwl_horizon_error takes host records; the _dev form reads device records in place on
 * `stream`; both wait for the stream once, at the end.
 * stpwl_horizon_plan answers on the host (no GPU) for a model of P points, r = n_x / 2, n_u inputs, n_z outputs and velocity weight w_v:
 * the windows W, the windows of a block and the blocks (= workgroups), mode (0 the L2-fed step: the staged layout plus the accumulators
 * exceed the 160 KB of LDS; 1 the region's panel staged in LDS; 2 staged with the point table held in registers: w_v = 0, P <= 64,
 * r <= 32), the dynamic LDS of the launch, the launches (2) and the byte cap of x_pred.  Not offered: weighting-mode models, the
 * Koopman analogue (the SSM analogue is sssm_horizon_error), closed-loop prediction, error weights other than H. */
int stpwl_horizon_plan(int r, int n_u, int P, int n_z, double w_v, int64_t E, int64_t T, int horizon, int stride, int every,
                       int64_t *windows, int *block, int64_t *blocks, int *mode, int64_t *lds_bytes, int64_t *launches,
                       int64_t *pred_cap_bytes);
int stpwl_horizon_error(stpwl_t *h, const double *x, const double *u, int64_t E, int64_t T, int horizon, int stride, int every,
                        double *sse, double *worst, int64_t *worst_at, int64_t *counts, double *final_norms, int32_t *status,
                        double *x_pred);
int stpwl_horizon_error_dev(stpwl_t *h, const double *x_dev, const double *u_dev, int64_t E, int64_t T, int horizon, int stride,
                            int every, double *sse, double *worst, int64_t *worst_at, int64_t *counts, double *final_norms,
                            int32_t *status, double *x_pred, void *stream);

/* SSM horizon error (csrc/ssm_horizon.hip): the k-step open-loop prediction error of an SSM model over records, read in place on the
 * device and started from the observer map exactly as the planners start -- the reference's model check
 * (examples/hardware/diamond_SSM.py:83-140 module_test) for every window start at once.
 * THE SSM HORIZON ERROR ("SSM horizon error", defines it):
 *   records     y (E x T x n_y) raw measurements as sssm_fit_add takes them, u (E x T x m), row i holds the input applied after y_i;
 *               `stride` s >= 1 keeps rows 0, s, 2s, ..; T' = the rows kept.
 *   model       the handle, a mode (SSSM_FE, SSSM_BE, SSSM_BIL at dt, or SSSM_DISCRETE_MAP), and the handle's z_ref.  Required:
 *               n_x == n_o == n_y, as sssm_rollout with outputs and the loops require.
 *   observed    xo_j = W_map(y_j - z_ref) = V phi_s(y_j - z_ref) for every kept row (the reference's SSMObserver).
 *   windows     starts at the kept rows j0 = 0, w, 2w, .. (`every` = w >= 1) of every episode while j0 + H <= T' - 1, H = `horizon`;
 *               numbered episode by episode in row order; an episode with T' <= H has none; W = 0 windows is refused (the window
 *               rule of stpwl_horizon_plan).
 *   prediction  xh_0 = xo_{j0}, or x_start (n_x) for every window when it is not NULL; xh_{k+1} = A_d xh_k + B_d u_{j0+k} + d_d with
 *               (A_d, B_d, d_d) linearised at (xh_k, u_{j0+k}) and discretised by the mode at dt; zh_k = C_map(xh_k) + z_ref.  The
 *               arithmetic is the plant step of sgusto_ssm_loop_advance: x_pred and z_pred are its X and Z + z_ref records bit for bit
 *               (not the bits of sssm_rollout, whose kernel sums in another order).
 *   errors      ez_k = zh_k - y_{j0+k} in the output space (NOT zero at k = 0: C_map(W_map(.)) is not the identity); ex_k = xh_k -
 *               xo_{j0+k} in the reduced space (exactly 0 at k = 0 without x_start).
 *   status      of a window: 0 ok; 1 some xh_k or zh_k is not finite; 2 some record row the window reads (y at j0 .. j0 + H, u at
 *               j0 .. j0 + H - 1) is not finite; 2 wins over 1.  Only status-0 windows enter the sums and the maxima.
 * Outputs (any but counts may be NULL): sse (2 x (H + 1)): sums of |ex_k|^2, then of |ez_k|^2; worst (2 x (H + 1)): the largest norm
 * (-1 when no window has status 0); worst_at (2 x (H + 1) x 2 int64): episode and row in the UNstrided record of the start of the window
 * that attains it, ties to the lowest window number (-1, -1: none); counts (3 int64): windows W, status-1 windows, status-2 windows;
 * final_norms (2 x W): |ex_H|_2, then |ez_H|_2 per window, NaN where status != 0; status (W); x_pred (W x (H + 1) x n_x), z_pred
 * (W x (H + 1) x n_o), x_obs (E x T' x n_x): the three together are refused above the byte cap that sssm_horizon_plan states.  A
 * window that left its loop at step k (the first xh_k or zh_k that is not finite) keeps its rows 0 .. k, the rows behind are NaN; a
 * status-2 window is not rolled out and all its rows are NaN.
 * Bits: no floating-point atomics; the windows are dealt to workgroups in fixed blocks by window number (`block` windows of one episode)
 * and the blocks' partial sums are joined in block order, so the result is a function of the records and parameters alone: not of
 * the CU count, a rerun gives the same bits, and device records give the bits of host arrays.  max is exact.
 * Limits (SRH_EINVAL before any device call, with the offending number): n_x <= 32, m <= 16, 1 <= H <= 1024, stride, every >= 1; the
 * continuous mode; the discrete map on a handle without rd_coeff; m > (n_x | 1) in be / bil (the B_d scratch panel of ssm::discretize); n_x != n_o or n_y != n_o; a launch above 160 KiB of LDS (with the
 * byte count).  sssm_horizon_error takes host records; the _dev form reads device records in place on `stream`; both wait for the
 * stream once, at the end.
 * sssm_horizon_plan answers on the host (no GPU) for a model of n_x states, n_u inputs, n_o outputs and the two orders, records of
 * n_y columns, a mode and whether the model has a discrete map: the windows W, the windows of a block and the blocks (= workgroups of
 * the window kernel), its dynamic LDS, the launches (3: observe, windows, join) and the byte cap of x_pred + z_pred + x_obs.
 * Not offered: the Koopman analogue, models with n_x != n_o, closed-loop prediction, error weights. */
int sssm_horizon_plan(int n_x, int n_u, int n_o, int n_y, int rom_order, int ssm_order, int mode, int has_discrete, int64_t E, int64_t T,
                      int horizon, int stride, int every, int64_t *windows, int *block, int64_t *blocks, int64_t *lds_bytes,
                      int64_t *launches, int64_t *pred_cap_bytes);
int sssm_horizon_error(sssm_t *h, int mode, double dt, const double *y, const double *u, int n_y, int64_t E, int64_t T, int horizon,
                       int stride, int every, const double *x_start, double *sse, double *worst, int64_t *worst_at, int64_t *counts,
                       double *final_norms, int32_t *status, double *x_pred, double *z_pred, double *x_obs);
int sssm_horizon_error_dev(sssm_t *h, int mode, double dt, const double *y_dev, const double *u_dev, int n_y, int64_t E, int64_t T,
                           int horizon, int stride, int every, const double *x_start, double *sse, double *worst, int64_t *worst_at,
                           int64_t *counts, double *final_norms, int32_t *status, double *x_pred, double *z_pred, double *x_obs,
                           void *stream);

/* =====================================================================================================
 * ROMPC baseline. reference: sofacontrol/baselines/rompc/rompc.py:57-89, rompc/observer.py:30-46, rompc_utils.py:52-53
 * `batch` independent loops on one linear reduced model (problem-major arrays everywhere).  One control step is
 *   u     = u_given                                   (start-up, rompc.py:69-70; or observer.update(u, y) on its own)
 *   u     = ubar + K (x_hat - xbar)                   (rompc.py:79)
 *   x_hat <- A x_hat + B u + d + L ((y - y_ref) - C x_hat)                          (observer.py:37-40)
 *   z     = H x_hat + z_ref, or C x_hat + y_ref when H is NULL (then n_z = n_y)     (observer.py:42-46)
 * FOLDED FORM: the device holds F = A_d - L C, formed on the host at srompc_create / srompc_set_gains, and evaluates
 * x_hat <- [F | B | L] [x_hat ; u ; y - y_ref] + d.  f64 throughout; a workgroup owns 16 problems, stages the constants in
 * LDS once and forms the products on v_mfma_f64_16x16x4_f64 (a problem gives the same bits alone and inside any batch).
 * Limits: n_x, n_u, n_y, n_z <= 128 each, and [F B L], K, the output map and the tile must fit 160 KB of LDS -- n_x = 80,
 * n_u = 16, n_y = 64, n_z = 16 fits (152 KB); the same without H (z = C x + y_ref, 64 rows) does not.  What does not fit is
 * refused by srompc_create with SRH_EINVAL.  K NULL: zeros.  Every call ends with the handle's stream drained.
 * ===================================================================================================== */
typedef struct srompc srompc_t;
int srompc_create(srompc_t **out, int64_t batch, int n_x, int n_u, int n_y, int n_z, const double *A_d, const double *B_d,
                  const double *d_d, const double *C, const double *y_ref, const double *H, const double *z_ref, const double *K,
                  const double *L);
int srompc_destroy(srompc_t *h);
int srompc_set_gains(srompc_t *h, const double *K, const double *L);      /* K (n_u x n_x), L (n_x x n_y); NULL keeps */
int srompc_set_state(srompc_t *h, const double *x);                       /* batch x n_x */
int srompc_get_state(srompc_t *h, double *x, double *z);                  /* either may be NULL */
/* observer.initialize (observer.py:30-35): x_hat = V^T (x_full - x_ref) by srom_project_dev straight into the estimate;
 * x_full (batch x 2 n_f), the basis must give 2 r = n_x.  x_out, z_out optional. */
int srompc_initialize(srompc_t *h, srom_t *rom, const double *x_full, double *x_out, double *z_out);
/* One control step: [x_full != NULL: initialize first] -> u (u_given, or the feedback on ubar (batch x n_u), xbar (batch x n_x))
 * -> observer update with y (batch x n_y, the full-order measurement) -> z.  One launch sequence on the handle's stream, one
 * copy back of (u, x_hat, z) and ONE blocking wait; inputs and results go through the handle's pinned blocks (no allocation,
 * except the full-state block at the first x_full call).  Outputs are optional. */
int srompc_step(srompc_t *h, srom_t *rom, const double *x_full, const double *u_given, const double *ubar, const double *xbar,
                const double *y, double *u_out, double *x_out, double *z_out);
/* T steps of the same recursion over a record in one launch: Y (T x batch x n_y), and U_given (T x batch x n_u) or
 * Ubar (T x batch x n_u) / Xbar (T x batch x n_x).  The time loop runs inside the kernel, the estimate tile stays in LDS,
 * Y[t] is streamed.  U_out / X_out / Z_out (T x batch x .) optional; the estimate ends at X_out[T - 1]. */
int srompc_replay(srompc_t *h, int T, const double *Y, const double *U_given, const double *Ubar, const double *Xbar,
                  double *U_out, double *X_out, double *Z_out);
/* steps taken, and the blocking host waits of the last initialize / step / replay call */
int srompc_stats(srompc_t *h, int64_t *steps, int64_t *waits_last_step);
/* For probes: srompc_set_timing(h, 1) brackets every following initialize / step / replay / get_state with HIP events on the
 * handle's stream; srompc_last_device_ms gives the last call's device-side duration, first enqueue to last copy (-1: none). */
int srompc_set_timing(srompc_t *h, int on);
int srompc_last_device_ms(srompc_t *h, double *ms);

/* Batched closed loop of the ROMPC baseline (csrc/rompc_loop.hip; reference rompc.py:57-141, observer.py:37-40, baselines/ros.py:202-235):
 * every problem b of the controller handle's batch is its own loop, resident on the device, ONE host wait per run.  B members, controller
 * step dt_sim, QP horizon N at dt_mpc, n_replan sub-steps per period (n_replan dt_sim <= N dt_mpc); period p starts at t_p = t_start +
 * p n_replan dt_sim (sgusto_loop_schedule).
 *   request   x0_p = x_hat0 of the reset (p = 0), else the previous plan's states interpolated at tau = n_replan dt_sim (interval
 *             j = min(int(tau / dt_mpc), N - 1), theta = (tau - j dt_mpc) / dt_mpc); targets: the window at (t_p + phase_b) + dt_mpc k,
 *             zf its last row when the cost has Qzf, u_des N rows
 *   solve     the trust-region-free QP with constant (A_mpc, B_mpc, d_mpc), all members in one launch, the horizon tiled once
 *   chain     row 0 of the plan's states <- x0_p; a member whose QP status is non-zero gets the previous plan moved up one row with its
 *             last row held (ros.py:223-227), in period 0 x0_0 in every state row and zero inputs; the status is recorded, the loop goes on
 *   sub-steps s = 0..n_replan-1 at tau = s dt_sim, (j_s, theta_s) of the schedule, ubar_s / xbar_s = lo + theta (hi - lo), the input held
 *             over the last interval, ONE launch for all of them:
 *               y_s       = (C x_s + y_ref) + v_s
 *               u_s       = ubar_s + K (x_hat_s - xbar_s)                                             (rompc.py:79)
 *               x_hat_s+1 = [F | B | L] [x_hat_s ; u_s ; y_s - y_ref] + d, F = A - L C                 (the constants of the srompc_t handle)
 *               x_s+1     = A_p[i] x_s + B_p[i] u_s + d_p[i] (+ w_s), i the plant's nearest point to x_s, or read from X_plant
 * Not offered: the start-up phase before t_delay, the full-order state and its projection, input clipping, dU rows, input_nullspace.
 * The batch is the controller's.  The loop reads the controller's gains and model at every reset and keeps its estimate in the
 * controller's own buffer on the loop's stream: do not step the controller elsewhere between a reset and the end of the runs that follow.
 * create refuses (with a message): a plant whose n_x or n_u differ from the controller's, n_u > 16, n_x > 128, a QP with a trust region
 * or dU rows or beyond the limits of slocp_plan_create, n_replan dt_sim > N dt_mpc, an advance kernel beyond 160 KiB of LDS.  The
 * controller and the plant must outlive the loop. */
typedef struct srompc_loop srompc_loop_t;
/* A_mpc (n_x x n_x), B_mpc (n_x x n_u), d_mpc (n_x): the QP's model at dt_mpc; plant: pre-discretised at dt_sim */
int srompc_loop_create(srompc_loop_t **out, srompc_t *ctrl, const slocp_problem *prob, const double *A_mpc, const double *B_mpc,
                       const double *d_mpc, double dt_mpc, stpwl_t *plant /* NULL: replay only */, double dt_sim, int n_replan,
                       int64_t max_steps_per_run);
int srompc_loop_destroy(srompc_loop_t *h);
/* t (T, increasing), z (T x n_z of the QP), u_des (T x n_u) or NULL, phase (batch) or NULL = zeros */
int srompc_loop_set_target(srompc_loop_t *h, int T, const double *t, const double *z, const double *u_des, const double *phase);
/* x0 (batch x n_x) plant states at the first solve, x_hat0 (batch x n_x) the estimates there */
int srompc_loop_reset(srompc_loop_t *h, const double *x0, const double *x_hat0 /* NULL: x0 */, double t_start);
/* `periods` periods (prepare -> solve -> chain -> advance each) on the handle's stream, the records copied back once, ONE blocking wait.
 * W (periods x n_replan x batch x n_x), V (periods x n_replan x batch x n_y) or NULL; X_plant (batch x (S + 1) x n_x) or NULL: the plant's
 * states are read from it (row 0 is where the run starts and is not read; W is then not used).  With S = periods n_replan: X, XH, Xbar
 * (batch x (S + 1) x n_x), Z (batch x (S + 1) x n_z of the controller; H x without z_ref), Y (batch x S x n_y), U, Ubar (batch x S x n_u);
 * row 0 = where the run started; the last row of Xbar is the next request's x0; J, status, iters (periods x batch). */
int srompc_loop_run(srompc_loop_t *h, int periods, const double *W, const double *V, const double *X_plant, double *X, double *XH, double *Y,
                    double *Z, double *U, double *Ubar, double *Xbar, double *J, int32_t *status, int32_t *iters);      /* any record may be NULL */
/* The solver inputs / the plan (after the chain fix-up) of the last period; any may be NULL */
int srompc_loop_last_inputs(srompc_loop_t *h, double *x0, double *z, double *zf, double *u_des);
int srompc_loop_last_plan(srompc_loop_t *h, double *xopt, double *uopt);
int srompc_loop_stats(srompc_loop_t *h, int64_t *steps, int64_t *waits_last_run);
/* The chain kernel alone on host arrays: the previous plan (NULL when first), the QP's answer xopt (batch x (N+1) x n_x), uopt (batch x N
 * x n_u), the request's x0 (batch x n_x), status (batch) -> the plan after the fix-up and x0_next (batch x n_x). */
int srompc_loop_chain(srompc_loop_t *h, const double *xopt_prev, const double *uopt_prev, const double *xopt, const double *uopt, const double *x0,
                      const int32_t *status, int first, double *xopt_out, double *uopt_out, double *x0_next);
/* The advance kernel alone on host arrays: plans, x, x_hat (batch x n_x), W (n_replan x batch x n_x) / V (n_replan x batch x n_y) or NULL,
 * X_plant (batch x (n_replan + 1) x n_x) or NULL -> after every sub-step X, XH (batch x n_replan x n_x), Z (batch x n_replan x n_z); of
 * every sub-step Y (batch x n_replan x n_y), U, Ubar (batch x n_replan x n_u), Xbar (batch x n_replan x n_x). */
int srompc_loop_advance(srompc_loop_t *h, const double *xopt, const double *uopt, const double *x, const double *x_hat, const double *W,
                        const double *V, const double *X_plant, double *X, double *XH, double *Y, double *Z, double *U, double *Ubar, double *Xbar);

/* =====================================================================================================
 * Batched closed-loop Koopman MPC resident on the device (csrc/koopman_loop.hip).  reference: sofacontrol/baselines/koopman/koopman.py:
 * 75-170 (compute_policy, evaluate), koopman_utils.py:16-47 (add_measurement, get_zeta), baselines/ros.py:202-235 (the MPC node and its
 * failure shift).  Every problem of an skoop_t handle's batch is its own loop.  THE POLICY: controller step Ts (the model's), simulation
 * step dt_sim with Ts = r dt_sim, r an integer >= 1; rollout_horizon = rh controller steps per period (rh <= N), n_keep = rh r sub-steps;
 * period p starts at t_p = t_start + p n_keep dt_sim (sgusto_loop_schedule, t_k only).
 *   reset     the ring of every member <- the `delays` older raw samples (y_hist, u_hist), oldest first, then the sample at the first
 *             solve: y_0 = (C x0 + y_ref) + v0 (or y0 given when there is no plant) pushed with u_prev0 (add_measurement(y, u_prev) in
 *             front of the first compute_policy); row 0 of the Y record is y_0
 *   request   x0_p = W psi(zeta) of the ring as it stands (the ring lift of skoop_ring_lift_dev); targets: the window at
 *             (t_p + phase_b) + Ts k, zf its last row when the cost has Qzf, u_des N rows
 *   solve     the trust-region-free QP on the constant (A, B), d = 0, all members in one launch, the horizon tiled once
 *   fix-up    a member whose QP status is non-zero goes on with the previous plan moved up ONE row, its last row held (ros.py:223-227,
 *             whatever rh is); in period 0 x0 in every state row and the scaled-down u0 in every input row; the status is recorded
 *   sub-steps s = 0..n_keep-1, ONE launch for all of them:
 *               u_s     = uopt[s / r] * u_factor + u_offset            (scale_up of the plan row of the controller step that has fired)
 *               x_s+1   = A_p[i] x_s + B_p[i] u_s + d_p[i] (+ w_s), i the plant's nearest point to x_s
 *               y_s+1   = (C x_s+1 + y_ref) + v_s, or read from Y_plant
 *               with a Y (skoop_loop_set_reproject): y_s+1 outside Y is replaced by its projection (koopman.py:150-151), with a plant and
 *                       in replay alike; the sample's status word (spoly_project_status) is recorded, -1 / -2 use the raw sample
 *               push (y_s+1 as used, u_s) -- with U_applied: (y_s+1, U_applied_s) -- scaled down, into the member's ring
 * Not offered: the start-up phase before t_delay, projecting the y_hist rows, input clipping, dU rows, input_nullspace,
 * nonlinear_observer, weighting-mode plants, the lifted model as its own plant.  The reference reads its input tape at its own knots,
 * so input_hold changes nothing and is not a parameter.
 * The loop works on the skoop_t handle's ring and advances its head and count: do not push to the handle elsewhere between a reset and
 * the end of the runs that follow.  create refuses (with a message): n_lift > 96, n_u > 16, a plant with n_x > 128 or n_u != the
 * model's, a plant without C or y_ref, a QP with a trust region or dU rows or whose n_x is not the lift's width,
 * |Ts / dt_sim - round(Ts / dt_sim)| > 1e-9, rollout_horizon outside 1..N, an advance kernel beyond 160 KiB of LDS.  The lift handle and
 * the plant must outlive the loop.
 * ===================================================================================================== */
typedef struct skoop_loop skoop_loop_t;
/* A (n_lift x n_lift), B (n_lift x n_u): the lifted model at Ts; plant: pre-discretised at dt_sim; C (n_y x n_plant), y_ref (n_y): the
 * plant's measurement (NULL without a plant); u0 (n_u) raw, NULL: zeros */
int skoop_loop_create(skoop_loop_t **out, skoop_t *h, const slocp_problem *prob, const double *A, const double *B, double Ts,
                      stpwl_t *plant /* NULL: replay only */, const double *C, const double *y_ref, const double *u0, double dt_sim,
                      int rollout_horizon, int64_t max_steps_per_run);
int skoop_loop_destroy(skoop_loop_t *h);
/* t (T, increasing), z (T x n_z of the QP), u_des (T x n_u, scaled down as the QP's inputs are) or NULL, phase (batch) or NULL = zeros */
int skoop_loop_set_target(skoop_loop_t *h, int T, const double *t, const double *z, const double *u_des, const double *phase);
/* x0 (batch x n_plant) plant states at the first solve, or y0 (batch x n_y) without a plant; y_hist (batch x delays x n_y), u_hist
 * (batch x delays x n_u) raw, oldest first (NULL when delays = 0); u_prev0 (batch x n_u) raw, NULL: u0; v0 (batch x n_y) or NULL */
int skoop_loop_reset(skoop_loop_t *h, const double *x0, const double *y0, const double *y_hist, const double *u_hist,
                     const double *u_prev0, const double *v0, double t_start);
/* `periods` periods (prepare -> lift -> solve -> fix-up -> advance each) on the handle's stream, the records copied back once, ONE
 * blocking wait.  W (periods x n_keep x batch x n_plant), V (periods x n_keep x batch x n_y) or NULL; Y_plant (batch x (S + 1) x n_y) or
 * NULL: the measurements are read from it (row 0 is where the run starts and is not read); U_applied (batch x S x n_u) or NULL: the
 * inputs pushed into the ring.  With S = periods n_keep: X (batch x (S + 1) x n_plant), Y (batch x (S + 1) x n_y), U (batch x S x n_u),
 * all raw, row 0 = where the run started; Xlift (periods x batch x n_lift) the requests; J, status, iters (periods x batch). */
int skoop_loop_run(skoop_loop_t *h, int periods, const double *W, const double *V, const double *Y_plant, const double *U_applied,
                   double *X, double *Y, double *U, double *Xlift, double *J, int32_t *status, int32_t *iters);   /* any record may be NULL */
/* The solver inputs / the plan (after the fix-up) of the last period; any may be NULL */
int skoop_loop_last_inputs(skoop_loop_t *h, double *x0, double *z, double *zf, double *u_des);
int skoop_loop_last_plan(skoop_loop_t *h, double *xopt, double *uopt);
int skoop_loop_stats(skoop_loop_t *h, int64_t *steps, int64_t *waits_last_run);
/* The fix-up kernel alone on host arrays: the previous plan (NULL when first), the QP's answer xopt (batch x (N+1) x n_lift), uopt
 * (batch x N x n_u), the request's x0 (batch x n_lift), status (batch) -> the plan after the fix-up. */
int skoop_loop_fixup(skoop_loop_t *h, const double *xopt_prev, const double *uopt_prev, const double *xopt, const double *uopt,
                     const double *x0, const int32_t *status, int first, double *xopt_out, double *uopt_out);
/* The advance kernel alone: plans uopt (batch x N x n_u), plant states x (batch x n_plant; NULL without a plant), W (n_keep x batch x
 * n_plant) / V (n_keep x batch x n_y) or NULL, Y_plant (batch x (n_keep + 1) x n_y), U_applied (batch x n_keep x n_u) or NULL -> after
 * every sub-step X (batch x n_keep x n_plant; NULL without a plant), Y (batch x n_keep x n_y), of every sub-step U (batch x n_keep x
 * n_u) and the plant's point idx (batch x n_keep; -1 without a plant).  It pushes into the lift handle's ring as it stands and advances
 * its head and count; the loop needs a reset before its next run. */
int skoop_loop_advance(skoop_loop_t *h, const double *uopt, const double *x, const double *W, const double *V, const double *Y_plant,
                       const double *U_applied, double *X, double *Y, double *U, int32_t *idx);
/* The admissible set of the measurements, Y = {y : A y <= b}, A (rows x n_y) row-major: from the next reset on every sample -- y_0 of
 * the reset included, the y_hist rows not -- is projected onto Y before it enters the ring.  n_y <= 16, rows <= 64, A and b finite
 * (refused with the numbers).  A = NULL or b = NULL removes Y.  The loop needs a reset behind either. */
int skoop_loop_set_reproject(skoop_loop_t *h, const double *A, const double *b, int rows);
/* skoop_loop_run with the two records of the re-projection: Y_used (batch x (S + 1) x n_y) the samples as the ring received them, proj
 * (batch x (S + 1)) their status words (spoly_project_status); row 0 = where the run started.  Y stays the raw measurement. */
int skoop_loop_run_reprojected(skoop_loop_t *h, int periods, const double *W, const double *V, const double *Y_plant, const double *U_applied,
                               double *X, double *Y, double *U, double *Xlift, double *J, int32_t *status, int32_t *iters, double *Y_used,
                               int32_t *proj);
/* skoop_loop_advance of a loop with a Y: also Y_used (batch x n_keep x n_y) and proj (batch x n_keep) of every sub-step */
int skoop_loop_advance_reprojected(skoop_loop_t *h, const double *uopt, const double *x, const double *W, const double *V, const double *Y_plant,
                                   const double *U_applied, double *X, double *Y, double *U, int32_t *idx, double *Y_used, int32_t *proj);

/* =====================================================================================================
 * Batched closed loop of the iLQR controller (tpwl.controllers.ilqr / TrajTracking), resident on the device.
 * reference: sofacontrol/tpwl/controllers.py:199-215, examples/diamond/diamond.py:318-389 (run_ilqr)
 * `batch` members, each with a plant state, an optional estimate, a per-step policy x_bar ((N+1) x n_x), u_bar (N x n_u),
 * K (N x n_u x n_x) and a held input.  Controller step dt = r dt_sim; controller step j fires at simulation step j r since the last
 * reset and reads policy row rows[j] (silqr_loop_set_rows: the host's table int(round(j dt, 4) / dt); default rows[j] = j).  A step
 * whose row is outside 0 .. N-1, or beyond the table, applies the idle input u0.  One simulation step s:
 *   1. if s % r == 0: u = u_bar[row] + K[row] (xl - x_bar[row]), xl the estimate with an observer, else the plant state; else u is held
 *   2. x <- d_d[i] + A_d[i] x + B_d[i] u (+ w_s), i the plant's nearest point to x, tables at dt_sim
 *   3. z = H x (the plant's output map)
 *   4. with an observer: y = (C x + y_ref) + v_s, then one step of every filter with (u, y)
 * Without an observer all steps of a run are one launch; with one, a step is advance -> filter -> record.  A run is one launch sequence
 * on the handle's stream and ONE host wait; the held input and the step counter live in the handle.  create refuses (with a message):
 * n_u > 16, a plant with n_x > 128, without tables at dt_sim or without an output map, a plan whose n_x, n_u, N or batch differ.
 * Not offered: SSM plants or plans, weighting-mode plants, input clipping, re-planning during a run, the start-up phase before
 * t_delay.  The plan, the plant and the observer must outlive the loop.
 * ===================================================================================================== */
typedef struct silqr_loop silqr_loop_t;
int silqr_loop_create(silqr_loop_t **out, silqr_plan_t *plan /* NULL: uploaded policies only */, stpwl_t *plant, int N, int r, int64_t batch,
                      int64_t max_steps_per_run);
int silqr_loop_destroy(silqr_loop_t *h);
/* shared != 0: x_bar ((N+1) x n_x), u_bar (N x n_u), K (N x n_u x n_x) for all members; else (batch x ...) each */
int silqr_loop_set_policy(silqr_loop_t *h, const double *x_bar, const double *u_bar, const double *K, int shared);
/* rows (count): the policy row of controller step j; a value outside 0 .. N-1 (and every j >= count) means the idle input */
int silqr_loop_set_rows(silqr_loop_t *h, const int32_t *rows, int64_t count);
int silqr_loop_set_idle_input(silqr_loop_t *h, const double *u0 /* (n_u) */);
/* a batched EKF of the same batch, n_x and n_u, its model pre-discretised at dt_sim; NULL detaches.  The loop needs a reset afterwards. */
int silqr_loop_set_observer(silqr_loop_t *h, sekf_batch_t *observer);
/* plant states x0 (batch x n_x); with an observer the estimates x_hat0 (NULL: x0) and Sigma0 are installed.  The step counter returns
 * to 0 and every member holds u0. */
int silqr_loop_reset(silqr_loop_t *h, const double *x0, const double *x_hat0);
/* One solve of the loop's plan from the belief where it stands on the device (the estimates with an observer, else the plant states),
 * on the loop's stream, no wait; its x, u, K become the policy in place.  u_warm (batch x N x n_u) or NULL. */
int silqr_loop_plan(silqr_loop_t *h, const double *u_warm);
/* `steps` simulation steps from where the handle stands.  W (steps x batch x n_x), V (steps x batch x n_y) or NULL.  Records: X (batch x
 * (steps + 1) x n_x) or NULL, Z (batch x (steps + 1) x n_z), row 0 = where the run started; U (batch x steps x n_u); with an observer
 * Xhat (batch x (steps + 1) x n_x), Y (batch x steps x n_y) and ekf_status (batch: the OR of the run's filter statuses), else NULL. */
int silqr_loop_run(silqr_loop_t *h, int64_t steps, const double *W, const double *V, double *X, double *Z, double *U, double *Xhat, double *Y,
                   int32_t *ekf_status);
/* The policy in use, in the shape it was installed (*shared says which); any may be NULL */
int silqr_loop_last_policy(silqr_loop_t *h, double *x_bar, double *u_bar, double *K, int *shared);
/* cost and iterations (batch each) of the plan's last solve */
int silqr_loop_plan_info(silqr_loop_t *h, double *cost, int32_t *iters);
int silqr_loop_stats(silqr_loop_t *h, int64_t *steps, int64_t *waits_last_run);
/* The advance kernel alone (no observer) under the policy in use: plant states x (batch x n_x), held inputs u_held (batch x n_u; NULL:
 * u0), `steps` steps with the step counter starting at step0 -> X (batch x steps x n_x), Z, U and the plant's picks idx (batch x steps,
 * or NULL).  The handle's own state is not touched. */
int silqr_loop_advance(silqr_loop_t *h, const double *x, const double *u_held, int64_t steps, int64_t step0, const double *W, double *X,
                       double *Z, double *U, int32_t *idx);

#ifdef __cplusplus
}
#endif
#endif /* SOFACONTROL_HIP_H */
