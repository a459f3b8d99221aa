/*
 * tritd.h — C ABI of libtritd.so, the MI355X-native TriTD-ADMM solver.
 *
 * Drop-in boundary for the reference call surface
 *     [A,B,C,O,errHist] = triple_decomp_ADMM(D, r, opts)
 * (fast_robust_triple_tensor/triple_decomp_ADMM.m:1, called at
 *  traffic_triple_comparison.m:55 and — as triple_decomp_ADMM_outlier — at
 *  video_triple_comparison.m:54), plus the L1 primitives the drivers and the
 * north star name (triple_product.m:1, unfold.m:1, soft_threshold.m:1,
 * buildF.m:1, buildG.m:1, buildH.m:1).
 *
 * Conventions
 *  - Plain pointers and sizes only; no framework types.
 *  - All host arrays are MATLAB column-major: X(i,j,t) at i + n1*(j + n2*t).
 *  - Factors use the reference shapes: A (n1,r,r), B (r,n2,r), C (r,r,n3).
 *  - Functions named tritd_dev_* take DEVICE pointers and a hipStream_t
 *    (passed as void*, NULL = default stream) and do not synchronise, except
 *    the metric forms, which return host scalars (evaluate, quality).
 *  - Every function returns a tritd_status; on error the message is available
 *    from tritd_last_error() (thread-local).
 *  - Inputs are never written (MATLAB shares mxArrays copy-on-write).
 */
#ifndef TRITD_H
#define TRITD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    TRITD_OK = 0,
    TRITD_ERR_ARG = 1,         /* bad shape / pointer / mode (unfold.m:12 'Mode must be 1, 2, or 3.') */
    TRITD_ERR_OPTS = 2,        /* missing opts field (triple_decomp_ADMM.m:16-20) */
    TRITD_ERR_HIP = 3,         /* HIP runtime error */
    TRITD_ERR_RCCL = 4,        /* RCCL error */
    TRITD_ERR_NOMEM = 5,       /* device allocation failed */
    TRITD_ERR_NODEV = 6,       /* no usable gfx950 device */
    TRITD_ERR_UNSUPPORTED = 7, /* rank / dtype outside the built kernels */
    TRITD_ERR_STATE = 8        /* call order / session state */
} tritd_status;

/* opts struct of triple_decomp_ADMM.m:16-20.  `present` is a bitmask of the
 * TRITD_OPT_* fields the caller actually set; a missing required field is
 * reported exactly like MATLAB's "Reference to non-existent field 'x'."
 * Extra reference-driver fields (alphaA, alphaB, origin —
 * traffic_triple_comparison.m:48-51) are ignored by the reference and have
 * no slot here. */
enum {
    TRITD_OPT_MU = 1u << 0,
    TRITD_OPT_RHO = 1u << 1,
    TRITD_OPT_LAMBDA = 1u << 2,
    TRITD_OPT_LAMBDA2 = 1u << 3,
    TRITD_OPT_MAXITER = 1u << 4,
    TRITD_OPT_TOL = 1u << 5,
    TRITD_OPT_DISP = 1u << 6,
    TRITD_OPT_ALL = 0x7fu
};

typedef struct {
    double mu;        /* opts.mu      (muL = muO = mu, :16-17) */
    double rho;       /* opts.rho     (rhoL = rhoO = rho) */
    double lambda;    /* opts.lambda  (E soft-threshold weight, :47) */
    double lambda2;   /* opts.lambda2 (ridge of update_A/update_B, :34-35) */
    double tol;       /* opts.tol     (relative-change stop, :63) */
    int32_t maxIter;  /* opts.maxIter */
    int32_t disp;     /* opts.disp    (print every 10 iterations, :60-62) */
    uint32_t present; /* TRITD_OPT_* bitmask */
    uint32_t model;   /* opts.model (not read by the reference): TRITD_MODEL_CP (0, the executed
                         rank-r^2 CP builders, fast_robust_triple_tensor/buildF.m) or TRITD_MODEL_QI
                         (1, Qi's 3-index triple product of origin_triple_tensor/buildF.m:2-6,
                         buildG.m:7-11, buildH.m:7-11; fp64, r <= 8; ADMM only) */
} tritd_opts;

enum { TRITD_MODEL_CP = 0, TRITD_MODEL_QI = 1 };

/* Line printer used for opts.disp ("Iter %d, errL=%.2e, errO=%.2e").
 * Default: stdout.  MEX gateways install mexPrintf here. */
typedef void (*tritd_print_fn)(const char* line, void* user);

/* Warning flags (bitmask).  Not errors: the call succeeded and its outputs
 * are valid, but they may differ from the reference's beyond rounding.
 * TRITD_FLAG_PINV_TOL: MATLAB's pinv (triple_decomp_ADMM.m:78,86,93;
 * triple_decomp_ALS.m:27,32,37) truncated an R x R ridge Gram here: a solve's
 * smallest pivot came within 1e3x of pinv's tolerance max(size)*eps(max sigma),
 * the device formed pinv of that Gram (Jacobi eigensolver with MATLAB's
 * tolerance) and it dropped at least one singular value. */
enum { TRITD_FLAG_PINV_TOL = 1u };

const char* tritd_version(void);
const char* tritd_last_error(void);
/* TRITD_FLAG_* of the last one-shot solve on this thread (tritd_admm_*,
 * tritd_admm_sharded_virtual_f64, tritd_als_*, tritd_ncvx_f64; OR over the
 * shards of a device set); 0 after a call that raised none, and after any
 * failed libtritd call. */
uint32_t tritd_last_flags(void);
void tritd_set_print_callback(tritd_print_fn fn, void* user);
/* Number of visible gfx950 devices (0 on a host without a GPU). */
tritd_status tritd_device_count(int32_t* count);

/* ---------------------------------------------------------------------------
 * One-shot drop-in solver.
 * Replaces fast_robust_triple_tensor/triple_decomp_ADMM.m:1-70.
 *   D       : n1*n2*n3 doubles (host)
 *   A0,B0,C0: initial factors in reference layout (the MATLAB wrapper draws
 *             them with randn in the order of :23 so the RNG stream matches)
 *   A,B,C   : outputs, reference layout
 *   O, E    : outputs, n1*n2*n3 (E is the 6th, extra output; either may be NULL, which also
 *             skips its device-to-host transfer)
 *   errHist : capacity maxIter; *iters receives k (errHist = errHist(1:k), :68)
 * Runs on `device`; device = -1 runs on the device set of tritd_set_devices
 * (the current device when none is set).
 * ------------------------------------------------------------------------- */
tritd_status tritd_admm_f64(const double* D, int64_t n1, int64_t n2, int64_t n3, int32_t r,
                            const tritd_opts* opts, const double* A0, const double* B0,
                            const double* C0, double* A, double* B, double* C, double* O,
                            double* E, double* errHist, int32_t* iters, int32_t device);
/* The same for D of MATLAB class single: O, E and
 * every array derived from D are single; A, B, C, errHist double (holding
 * the single-rounded values MATLAB's class rules produce).  r <= 16.
 * MATLAB: the wrapper passes single(D) here, mxSINGLE_CLASS outputs. */
tritd_status tritd_admm_f32(const float* D, int64_t n1, int64_t n2, int64_t n3, int32_t r,
                            const tritd_opts* opts, const double* A0, const double* B0,
                            const double* C0, double* A, double* B, double* C, float* O, float* E,
                            double* errHist, int32_t* iters, int32_t device);
/* Mask-aware form (fp64): fit the observed entries only.  `observed` is
 * n1*n2*n3 bytes laid out like D (host, column-major), nonzero = observed.
 * Unobserved entries of D are never read as data (any fill value, NaN
 * included): D <- observed .* D and normD = ||observed .* D|| before the loop
 * (:28), and in every iteration D~ = where(observed, D, L) stands for D in
 * :41, :50 and in the next iteration's :33.  O, E and the multipliers are then
 * exactly 0 at unobserved entries, the factor updates see the current model L
 * there, and errHist counts observed entries only.  observed == NULL behaves
 * as tritd_admm_f64; a mask with no true entry is TRITD_ERR_ARG.  device = -1
 * runs on the device set (mode-1 shards, one device repeated P times
 * included).  opts.model = TRITD_MODEL_QI is supported.
 *   NaN as missing: observed = TRITD_OBSERVED_NAN (below) means
 *   Omega = ~isnan(D), elementwise, and no mask array exists.  Any NaN counts
 *   as missing (either sign, any payload, quiet or signalling); +-Inf is data.
 *   The mask is taken from D on the device; every output is bit for bit that
 *   of the same call with the byte mask (uint8_t)!isnan(D).  Every `observed`
 *   parameter of this header accepts the constant, the holdout forms and the
 *   session creators (device-resident D, any leading dimension) included; a
 *   `holdout` array stays a byte mask.  The constant is never dereferenced and
 *   never offset (shards pass it through).  An all-NaN D is the mask with no
 *   true entry.  Without the constant a NaN in D is data and propagates. */
#define TRITD_OBSERVED_NAN ((const uint8_t*)(uintptr_t)1)
tritd_status tritd_admm_masked_f64(const double* D, const uint8_t* observed, int64_t n1, int64_t n2,
                                   int64_t n3, int32_t r, const tritd_opts* opts, const double* A0,
                                   const double* B0, const double* C0, double* A, double* B,
                                   double* C, double* O, double* E, double* errHist, int32_t* iters,
                                   int32_t device);
/* Held-out validation error, best iterate and early stopping for the masked
 * ADMM.  `observed` (Omega; NULL = all true) and `holdout` (H) are n1*n2*n3
 * bytes laid out like D, nonzero = true; patience >= 0; val_norm is 2 or 1.
 * observed may be TRITD_OBSERVED_NAN (tritd_admm_masked_f64).
 * Line numbers are fast_robust_triple_tensor/triple_decomp_ADMM.m's.
 *   Only H & Omega counts: a held-out flag at an unobserved entry is ignored,
 *   whatever D holds there (NaN and Inf included).
 *   The fit is exactly tritd_admm_masked_f64 with observed = Omega & ~H:
 *   D <- (Omega & ~H) .* D, normD (:28) is that tensor's norm, and the fused
 *   update sees the fit mask only.  With patience = 0, A, B, C, O, E, errHist
 *   and *iters are bit for bit those of that call.  O and E are exactly 0 at
 *   the held-out entries, as at the unobserved ones.
 *   With L_k = triple_product(A, B, C) of the factors AFTER the updates of
 *   iteration k (what the call would return if it ended at k):
 *     valHist(k)  = ||H .* Omega .* (D - L_k)|| / ||H .* Omega .* D||
 *     valHist1(k) = sum_{H & Omega} |D - L_k| / sum_{H & Omega} |D|
 *   Both are always computed and are truncated with errHist (:68).  (The
 *   held-out entries of a robust problem carry outliers too, and they dominate
 *   a squared score: valHist1 is the one to read there.)  The device takes L_k
 *   from T of iteration k+1, which the masked update leaves equal to L_k
 *   outside the fit mask.
 *   val_norm picks the history that drives the decisions: 2 valHist, 1 valHist1.
 *   best_iter = argmin_k of that history, the first minimum on a tie (a strict
 *   < against the running best, k = 1 always taken).  A_best, B_best, C_best
 *   are the factors after iteration best_iter, kept on the device: bit for bit
 *   the factors of the masked call with maxIter = best_iter.  O and E of the
 *   best iterate are NOT kept (a tensor copy per improvement is too dear):
 *   re-run the masked call with maxIter = best_iter for them.
 *   Early stop, patience = p > 0 only: after the stop test of :63 for
 *   iteration k, k - best_iter >= p stops the loop at k like a reference stop:
 *   k iterations are done and the outputs are those of iteration k.
 *   stop_reason: 0 ran to maxIter (or not stopped yet), 1 the test of :63,
 *   2 patience.
 *   TRITD_ERR_ARG: holdout == NULL, H & Omega empty, Omega & ~H empty,
 *   ||H .* Omega .* D|| = 0, patience < 0, val_norm not 1 or 2.  On a device
 *   set or with a communicator every shard refuses alike (the counts and norms
 *   are reduced at creation).  TRITD_ERR_UNSUPPORTED: opts.model =
 *   TRITD_MODEL_QI (and TRITD_SESSION_F32 for a session, as for any mask).
 * valHist and valHist1 have the capacity of errHist (maxIter); A_best, B_best,
 * C_best, valHist, valHist1, best_iter and stop_reason may be NULL.  device =
 * -1 runs on the device set as tritd_admm_masked_f64 does (the A rows of the
 * best iterate are shard-local, B and C replicated; every shard takes the same
 * decisions). */
tritd_status tritd_admm_holdout_f64(const double* D, const uint8_t* observed, const uint8_t* holdout,
                                    int64_t n1, int64_t n2, int64_t n3, int32_t r,
                                    const tritd_opts* opts, int32_t patience, int32_t val_norm,
                                    const double* A0, const double* B0, const double* C0, double* A,
                                    double* B, double* C, double* O, double* E, double* errHist,
                                    int32_t* iters, double* A_best, double* B_best, double* C_best,
                                    double* valHist, double* valHist1, int32_t* best_iter,
                                    int32_t* stop_reason, int32_t device);

/* ---------------------------------------------------------------------------
 * Sessions: the device-resident ADMM loop, steppable (bench), shardable
 * along mode 1 (multi-GPU).  A session owns a shard i in [i0, i1) of the
 * global n1 x n2 x n3 problem (i0 = 0, i1 = n1 for one GPU).
 * ------------------------------------------------------------------------- */
typedef struct tritd_session tritd_session;
typedef struct tritd_comm tritd_comm;

enum {
    TRITD_SESSION_D_ON_DEVICE = 1, /* D is a device pointer on `device` */
    TRITD_SESSION_F32 = 2,         /* D is float (class single): the fp32 data path */
    TRITD_SESSION_PROBE = 4        /* choose where the tensor pool lives by timing the fused
                                      update's access pattern on up to 16 candidate allocations
                                      (~5-10 % on that kernel; pays off over hundreds of
                                      iterations, so the one-shot calls never do it) */
};

/* D points at D(i0,0,0) (double, or float with TRITD_SESSION_F32); consecutive (j,t) fibres are ldD elements apart
 * (ldD = n1 for a full column-major tensor).  A0 is the FULL (n1,r,r)
 * initial A (rows i0..i1-1 are used); B0, C0 are full.  comm = NULL for a
 * single process/GPU. */
tritd_status tritd_session_create(tritd_session** out, int32_t device, const void* D, int64_t ldD,
                                  int64_t n1, int64_t n2, int64_t n3, int64_t i0, int64_t i1,
                                  int32_t r, const tritd_opts* opts, const double* A0,
                                  const double* B0, const double* C0, tritd_comm* comm,
                                  uint32_t flags);
/* tritd_session_create with a mask (see tritd_admm_masked_f64).  observed
 * points at the mask byte of D(i0,0,0); consecutive (j,t) fibres are ldD BYTES
 * apart (the mask has the shape and leading dimension of D, one byte per
 * element).  It is a device pointer exactly when TRITD_SESSION_D_ON_DEVICE is
 * set.  observed == NULL: as tritd_session_create.  With TRITD_SESSION_F32 a
 * mask is TRITD_ERR_UNSUPPORTED; a mask with no true entry in any shard is
 * TRITD_ERR_ARG (with a communicator: on every rank alike).  observed may be
 * TRITD_OBSERVED_NAN (tritd_admm_masked_f64), with a host or a device D. */
tritd_status tritd_session_create_masked(tritd_session** out, int32_t device, const void* D,
                                         const uint8_t* observed, int64_t ldD, int64_t n1,
                                         int64_t n2, int64_t n3, int64_t i0, int64_t i1, int32_t r,
                                         const tritd_opts* opts, const double* A0, const double* B0,
                                         const double* C0, tritd_comm* comm, uint32_t flags);
/* Whether the session was created with a mask, and the number of observed
 * entries of its shard (all of them without a mask).  Either may be NULL. */
tritd_status tritd_session_mask_info(tritd_session* s, int32_t* masked, int64_t* observed_count);
/* tritd_session_create_masked with a holdout mask (tritd_admm_holdout_f64):
 * holdout follows the conventions of observed (the mask byte of D(i0,0,0),
 * fibres ldD BYTES apart, a device pointer exactly when
 * TRITD_SESSION_D_ON_DEVICE is set); observed may be NULL (all true).  A run
 * after a patience stop is a no-op, like one after a stop of :63.  With a
 * communicator every rank creates a holdout session with the same patience
 * and val_norm (a mismatch is TRITD_ERR_ARG on every rank). */
tritd_status tritd_session_create_holdout(tritd_session** out, int32_t device, const void* D,
                                          const uint8_t* observed, const uint8_t* holdout,
                                          int64_t ldD, int64_t n1, int64_t n2, int64_t n3,
                                          int64_t i0, int64_t i1, int32_t r, const tritd_opts* opts,
                                          int32_t patience, int32_t val_norm, const double* A0,
                                          const double* B0, const double* C0, tritd_comm* comm,
                                          uint32_t flags);
/* The held-out entries (H & Omega) of the session's shard, and
 * ||H .* Omega .* D|| and sum |H .* Omega .* D| over all shards.  Any may be
 * NULL. */
tritd_status tritd_session_holdout_info(tritd_session* s, int64_t* count, double* norm,
                                        double* sum1);
/* valHist and valHist1 (as many entries as errHist has; capacity maxIter),
 * best_iter (0 before the first iteration) and stop_reason.  Any may be NULL.
 * Synchronises. */
tritd_status tritd_session_get_val(tritd_session* s, double* valHist, double* valHist1,
                                   int32_t* best_iter, int32_t* stop_reason);
/* The factors after iteration best_iter (A0, B0, C0 before any run), shaped
 * like those of tritd_session_get (A: the shard's rows).  Any may be NULL.
 * Synchronises. */
tritd_status tritd_session_get_best(tritd_session* s, double* A, double* B, double* C);
/* With tritd_session_set_timing(TRITD_TIMING_ALL): ms per timed iteration in
 * the score kernel, and from the end of the fused update to the end of the
 * iteration (score, reductions, finish, snapshot).  Either may be NULL.
 * These four are TRITD_ERR_STATE on a session without a holdout. */
tritd_status tritd_session_holdout_ms(tritd_session* s, double* score_ms, double* tail_ms);
/* Enqueue `iters` ADMM iterations (no host synchronisation unless opts.disp).
 * Iterations after the stop test of :63 fires, or beyond maxIter, are no-ops. */
tritd_status tritd_session_run(tritd_session* s, int32_t iters);
/* Wait for the enqueued work; report iterations completed and the stop flag. */
tritd_status tritd_session_sync(tritd_session* s, int32_t* iters_done, int32_t* stopped);
/* Copy results to the host.  A: full (n1,r,r) buffer, only rows i0..i1-1 are
 * written; B, C full; O, E: the shard, leading dimension ldOE (>= i1-i0);
 * errHist capacity maxIter.  Any pointer may be NULL. */
tritd_status tritd_session_get(tritd_session* s, double* A, double* B, double* C, double* O,
                               double* E, int64_t ldOE, double* errHist, int32_t* iters);
/* Driver RRE (traffic_triple_comparison.m:62-63,194-199) of the current
 * factors against a device-resident reference tensor X (same shard/ld as D):
 *   sum over the shard of (triple_product(A,B,C) - X)^2 and of X^2.
 * (Combine across ranks, then RRE = sqrt(num/den).) */
tritd_status tritd_session_rre_parts(tritd_session* s, const double* dX, int64_t ldX, double* num,
                                     double* den);
/* fp32 sessions (TRITD_SESSION_F32): O, E and the reference tensor are float. */
tritd_status tritd_session_get_f32(tritd_session* s, double* A, double* B, double* C, float* O,
                                   float* E, int64_t ldOE, double* errHist, int32_t* iters);
tritd_status tritd_session_rre_parts_f32(tritd_session* s, const float* dX, int64_t ldX,
                                         double* num, double* den);
/* Kernel-level timing of the dominant kernels over the last run (ms per
 * launch, HIP events on the session stream; 0 when timing is disabled). */
/* enable: 0 off; TRITD_TIMING_ALL (1): per-iteration events around the
 * iteration, K2 and K5; TRITD_TIMING_K5 (2): around K5 only (each event
 * record is a stream marker that widens the next kernel boundary by µs) */
enum { TRITD_TIMING_ALL = 1, TRITD_TIMING_K5 = 2 };
tritd_status tritd_session_set_timing(tritd_session* s, int32_t enable);
tritd_status tritd_session_kernel_ms(tritd_session* s, double* fused_update_ms, double* mode3_ms,
                                     double* iteration_ms, int32_t* samples);
/* All-reduce time of the timed iterations (TRITD_TIMING_ALL, a session with
 * a communicator): the mean ms per iteration spent between
 * issuing the iteration's all-reduces and their completion on the session
 * stream (waiting for the slowest rank included), and how many all-reduces
 * an iteration issued (0 without a communicator).  Per-rank breakdown of
 * bench.py's N > 1 line: iteration ms - all-reduce ms = compute. */
tritd_status tritd_session_comm_ms(tritd_session* s, double* allreduce_ms, int32_t* per_iteration);
/* Placement probe of the session's tensor pool: the probe
 * time (ms) of each candidate pool that was tried (up to cap entries) and
 * the index kept.  *n = 1 when probing was skipped. */
tritd_status tritd_session_probe(tritd_session* s, double* ms, int32_t cap, int32_t* n,
                                 int32_t* picked);
/* Compact-E counters: E tiles stored densely (more than 28
 * nonzeros of 256) summed over all fused-update launches so far, and the
 * number of tiles one launch covers. */
tritd_status tritd_session_counters(tritd_session* s, int64_t* dense_tiles_total,
                                    int64_t* tiles_per_launch);
/* Streaming profile of the session's fused update: dense
 * N-element streams per launch (6 = D, Y_L, Y_O read + Y_L, Y_O, T written;
 * 4 with the derived Y_O of the fp64 path) and compact-E slot accesses per
 * tile (2 = E read + written; 3 = E^(k), E^(k-1) read + E^(k+1) written). */
tritd_status tritd_session_k5_profile(tritd_session* s, int32_t* dense_streams,
                                      int32_t* slot_accesses);
/* TRITD_FLAG_* raised by this session's solves so far (read at each sync). */
tritd_status tritd_session_flags(tritd_session* s, uint32_t* flags);
void tritd_session_destroy(tritd_session* s);

/* ---------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, RCCL over xGMI.  Rank 0 creates the id,
 * the host side broadcasts its 128 bytes (e.g. torch.distributed), every
 * rank calls tritd_comm_create.
 * ------------------------------------------------------------------------- */
tritd_status tritd_comm_unique_id(void* id128);
tritd_status tritd_comm_create(tritd_comm** out, const void* id128, int32_t nranks, int32_t rank,
                               int32_t device);
/* Host transport: every all-reduce of a session using this comm drains the
 * session's stream, copies the buffer to the host and calls fn(buf, count, op,
 * user) (op 0 = sum, 1 = max; return 0 on success), then copies it back.  For
 * hosts that own a collective layer already (MPI, gloo) and for running the
 * multi-rank schedule with several ranks on one GPU (RCCL refuses a GPU twice
 * in one communicator).  tritd_comm_create (RCCL, device-side, asynchronous)
 * is the fast path. */
typedef int32_t (*tritd_allreduce_fn)(double* buf, int64_t count, int32_t op, void* user);
tritd_status tritd_comm_create_host(tritd_comm** out, tritd_allreduce_fn fn, void* user,
                                    int32_t nranks, int32_t rank, int32_t device);
void tritd_comm_destroy(tritd_comm* c);
/* What the communicator itself reports: for RCCL, ncclCommCount /
 * ncclCommUserRank read back from the communicator (so a caller can prove
 * RCCL saw every rank); for the host transport, the values it was created
 * with.  transport: 0 = RCCL, 1 = host. */
tritd_status tritd_comm_info(tritd_comm* c, int32_t* nranks, int32_t* rank, int32_t* transport);

/* Device set of the one-shot entry points (the MEX host
 * calls from its one thread).  With n > 1, tritd_admm_{f64,f32} (device =
 * -1) shard D along mode 1 over the set: the library runs one
 * session per shard with a communicator, each stepped by a library-owned
 * host thread (shard 0 on the calling thread, so disp prints stay there)
 * through the same fused two-all-reduce schedule as one process per GPU.
 * Distinct devices all-reduce over RCCL (communicators from ncclCommInitAll,
 * cached until the set changes or tritd_shutdown); one device repeated n
 * times runs n shards on it with an in-process all-reduce.  TRITD_SHOV=0
 * selects the phase-serial order driven from the calling thread instead.
 * n = 0 clears the set.  Replaces the reference's single-process CPU call
 * (triple_decomp_ADMM.m:1) for data that exceeds one GPU. */
tritd_status tritd_set_devices(const int32_t* devices, int32_t n);
/* Frees the cached communicators and clears the device set (mexAtExit). */
void tritd_shutdown(void);

/* Single-GPU rehearsal of the sharded path: `nshards` sessions on one device
 * whose all-reduces are summed on the device in shard order (the device set
 * {device} x nshards).  Used by the parity tests on a 1-GPU box. */
tritd_status tritd_admm_sharded_virtual_f64(const double* D, int64_t n1, int64_t n2, int64_t n3,
                                            int32_t r, const tritd_opts* opts, const double* A0,
                                            const double* B0, const double* C0, int32_t nshards,
                                            double* A, double* B, double* C, double* O, double* E,
                                            double* errHist, int32_t* iters, int32_t device);

/* ---------------------------------------------------------------------------
 * ALS variant: [A,B,C,errHist] = triple_decomp_ALS(X, r, opts)
 * (fast_robust_triple_tensor/triple_decomp_ALS.m:1-40).
 * Only opts.maxIter and opts.tol are read (:2-3): TRITD_OPT_MAXITER and
 * TRITD_OPT_TOL must be present, a missing one fails like MATLAB.  errHist(k)
 * = ||X - triple_product(A,B,C)||/||X|| is taken before the update of
 * iteration k; the stop test (:20) returns the factors of that iteration
 * un-updated, errHist = errHist(1:k).  Every mode uses the ridge 1e-9.  The
 * progress line "Iteration %d, relative error = %.4e" goes to the print
 * callback every 5 iterations (:17-19).  fp64, r <= 8.  device = -1 runs on
 * the device set of tritd_set_devices (mode-1 shards).
 * ------------------------------------------------------------------------- */
tritd_status tritd_als_f64(const double* X, int64_t n1, int64_t n2, int64_t n3, int32_t r,
                           const tritd_opts* opts, const double* A0, const double* B0,
                           const double* C0, double* A, double* B, double* C, double* errHist,
                           int32_t* iters, int32_t device);
/* Mask-aware form: fit the observed entries only.  `observed` is n1*n2*n3
 * bytes laid out like X (host, column-major), nonzero = observed.  Unobserved
 * entries of X are never read as data (any fill value, NaN and Inf included):
 * X <- observed .* X and Xnorm = ||observed .* X|| before the loop (:6), and in
 * iteration k X~ = where(observed, X, Xhat), with Xhat = triple_product(A,B,C)
 * of :15, stands for X in :16 and in all three updates of that iteration
 * (:25-38): errHist counts observed entries only and the updates see the
 * current model at the missing ones.  The stop test, the ridge 1e-9, the
 * update order and the progress line are unchanged; with every entry observed
 * every statement is the reference's.  observed == NULL behaves as
 * tritd_als_f64; a mask with no true entry is TRITD_ERR_ARG.  device = -1 runs
 * on the device set (mode-1 shards, one device repeated P times included). */
tritd_status tritd_als_masked_f64(const double* X, const uint8_t* observed, int64_t n1, int64_t n2,
                                  int64_t n3, int32_t r, const tritd_opts* opts, const double* A0,
                                  const double* B0, const double* C0, double* A, double* B,
                                  double* C, double* errHist, int32_t* iters, int32_t device);
/* Held-out validation error and early stopping for the masked ALS.
 * `observed` (Omega; NULL = all true) and `holdout` (H) are n1*n2*n3 bytes laid
 * out like X, nonzero = true; patience >= 0.  Only H & Omega counts: a held-out
 * flag at an unobserved entry is ignored, whatever X holds there (NaN
 * included).  Line numbers are fast_robust_triple_tensor/triple_decomp_ALS.m's.
 *   The fit is exactly tritd_als_masked_f64 with observed = Omega & ~H:
 *   Xnorm = ||(Omega & ~H) .* X|| (:6) and X~ = where(Omega & ~H, X, Xhat)
 *   stands for X in :16 and :25-38.  With patience = 0, A, B, C, errHist and
 *   *iters are bit for bit those of that call.
 *   valHist(k) = ||H .* Omega .* (X - Xhat)|| / ||H .* Omega .* X|| with the Xhat
 *   of :15 in iteration k: like errHist(k) it scores the factors iteration k
 *   started with, and it is truncated with errHist (:21).  It is summed in the
 *   fit kernel's own pass over X.
 *   best_iter = argmin_k valHist(k), the first minimum on a tie (a strict <
 *   against the running best, k = 1 always taken).  A_best, B_best, C_best are
 *   the factors iteration best_iter started with (best_iter = 1: A0, B0, C0
 *   exactly), kept on the device.
 *   Early stop, patience = p > 0 only: after the stop test of :20, if
 *   k - best_iter >= p the loop stops at k like a reference stop: the updates
 *   of k do not run and A, B, C are the factors of iteration k un-updated.
 *   stop_reason: 0 ran to maxIter (or not stopped yet), 1 the test of :20,
 *   2 patience.
 *   TRITD_ERR_ARG: H & Omega empty, Omega & ~H empty, ||H .* Omega .* X|| = 0,
 *   patience < 0, holdout == NULL.  On a device set or with a communicator
 *   every shard refuses alike (the counts and norms are reduced at creation).
 * valHist has the capacity of errHist (maxIter); A_best, B_best, C_best,
 * valHist, best_iter and stop_reason may be NULL.  device = -1 runs on the
 * device set as tritd_als_masked_f64 does (the A rows of the best iterate are
 * shard-local, B and C replicated; every shard takes the same decisions). */
tritd_status tritd_als_holdout_f64(const double* X, const uint8_t* observed, const uint8_t* holdout,
                                   int64_t n1, int64_t n2, int64_t n3, int32_t r,
                                   const tritd_opts* opts, int32_t patience, const double* A0,
                                   const double* B0, const double* C0, double* A, double* B,
                                   double* C, double* errHist, int32_t* iters, double* A_best,
                                   double* B_best, double* C_best, double* valHist,
                                   int32_t* best_iter, int32_t* stop_reason, int32_t device);
/* Steppable ALS session (bench, one process per GPU with comm; shard rows
 * [i0, i1) as for tritd_session_create; flags: TRITD_SESSION_D_ON_DEVICE).
 * quiet = 1 skips the every-5-iterations progress line (and its host
 * synchronisation). */
/* Nonconvex variant, fast_robust_triple_tensor/test.m:1-73 (the file's function
 * is named triple_decomp_ADMM_outlier(X, r, rho, lambda, gamma_A, epsilon, p, theta,
 * maxIter, tol)).  Outlier ADMM over Y = X - O with duals
 * Lambda, Gamma, while A, B, C follow an ALS on X (ridge 1e-12 + reweighted
 * shrink on A, 1e-9 on B, C).  errHist(k) = ||X - Y - O||/||X|| after the updates,
 * printed every iteration ("Iteration %d, relative error = %.4e"); on the stop
 * test errHist holds *iters entries and O is that of iteration *iters - 1
 * (the reference breaks before O = O_new).  X, O column-major n1 x n2 x n3;
 * factors as tritd_admm_f64; errHist capacity maxIter; fp64, r <= 8.
 * device < 0: the device set (tritd_set_devices) or the current device. */
tritd_status tritd_ncvx_f64(const double* X, int64_t n1, int64_t n2, int64_t n3, int32_t r,
                           double rho, double lambda, double gamma_A, double epsilon, double p,
                           double theta, int32_t maxIter, double tol, const double* A0,
                           const double* B0, const double* C0, double* A, double* B, double* C,
                           double* O, double* errHist, int32_t* iters, int32_t device);
/* Mask-aware form of tritd_ncvx_f64: fit the observed entries only.  `observed`
 * is n1*n2*n3 bytes laid out like X (host, column-major), nonzero = observed
 * (Omega below).  Line numbers are fast_robust_triple_tensor/test.m's.
 *   Before the loop X <- Omega .* X and Xnorm = ||Omega .* X|| (:21): the
 *   values of X at unobserved entries (0, NaN, +-Inf, sentinels) are never read
 *   as data.  In iteration k, after T = triple_product(A,B,C) (:35),
 *   X~ = where(Omega, X, T) stands for X.
 *   At an observed entry :36 (Y_new), :44 (O_new), :47 (Lambda), :48 (Gamma) and
 *   :62 (errHist) are the reference's statements in the reference's operator
 *   order.  At an unobserved entry their exact-arithmetic values for x = T,
 *   O = Lambda = Gamma = 0 are imposed, not computed ((T + rho T)/(1 + rho)
 *   rounds to something other than T): Y_new = T, O_new = 0, Lambda and Gamma
 *   keep their value (exactly 0 for every k), and the entry adds exactly 0 to
 *   errHist(k).  The returned O is exactly 0 where unobserved.
 *   The factor updates :49-51 (ridge 1e-12 + reweighted shrink on A, 1e-9 on B
 *   and C) take X~ for X, with T of the start of the iteration: an EM step per
 *   iteration, as tritd_als_masked_f64.
 *   Unchanged: the stop test :65-68, errHist = errHist(1:k), the returned O being
 *   that of iteration k-1 on a break (:71), the progress line of every iteration
 *   (:63).  With every entry observed the result is that of tritd_ncvx_f64 bit
 *   for bit; observed == NULL behaves as tritd_ncvx_f64; a mask with no true
 *   entry is TRITD_ERR_ARG.  device = -1 runs on the device set (mode-1 shards,
 *   one device repeated P times included; TRITD_SHOV=0: the phase-serial
 *   order). */
tritd_status tritd_ncvx_masked_f64(const double* X, const uint8_t* observed, int64_t n1, int64_t n2,
                                   int64_t n3, int32_t r, double rho, double lambda, double gamma_A,
                                   double epsilon, double p, double theta, int32_t maxIter,
                                   double tol, const double* A0, const double* B0, const double* C0,
                                   double* A, double* B, double* C, double* O, double* errHist,
                                   int32_t* iters, int32_t device);
/* Held-out validation error, best iterate and early stopping for the masked
 * nonconvex solver.  `observed` (Omega; NULL = all true) and `holdout` (H) are
 * n1*n2*n3 bytes laid out like X, nonzero = true; patience >= 0; val_norm is 2
 * or 1.  Only H & Omega counts: a held-out flag at an unobserved entry is
 * ignored, whatever X holds there (NaN and Inf included).  Line numbers are
 * fast_robust_triple_tensor/test.m's.
 *   The fit is exactly tritd_ncvx_masked_f64 with observed = Omega & ~H.  With
 *   patience = 0, A, B, C, O, errHist and *iters are bit for bit those of that
 *   call.  O, Lambda and Gamma are exactly 0 at held-out entries, as at
 *   unobserved ones.
 *   With T_k the product of :35 in iteration k,
 *     valHist(k)  = ||H .* Omega .* (X - T_k)|| / ||H .* Omega .* X||,
 *     valHist1(k) = sum_{H & Omega} |X - T_k| / sum_{H & Omega} |X|.
 *   Both are always computed, and truncated with errHist (:66).  They score the
 *   factors iteration k started with.  The l1 form exists because held-out
 *   entries of a robust problem carry outliers, which dominate the l2 form.
 *   val_norm picks the history that drives the decisions below.
 *   best_iter is the first minimum of that history (a strict < against the
 *   running best, k = 1 always taken).  A_best, B_best, C_best are the factors
 *   iteration best_iter started with (best_iter = 1: A0, B0, C0 exactly), kept
 *   on the device; they are bit for bit the factors of the masked call run
 *   best_iter - 1 iterations.  O of the best iterate is not kept.
 *   Early stop, patience = p > 0 only: after the stop test of :65-68 for
 *   iteration k, k - best_iter >= p stops the loop at k exactly like a reference
 *   break: the updates of k have run, O is that of k-1 (:71), and both
 *   histories have k entries.
 *   stop_reason: 0 ran to maxIter (or not stopped yet), 1 the test of :65,
 *   2 patience.
 *   TRITD_ERR_ARG: holdout == NULL, H & Omega empty, Omega & ~H empty,
 *   ||H .* Omega .* X|| = 0, patience < 0, val_norm not 1 or 2, rho == 0.  On a
 *   device set or with a communicator every shard refuses alike (the counts and
 *   sums are reduced at creation).  TRITD_ERR_UNSUPPORTED: r > 8.
 * valHist and valHist1 have the capacity of errHist (maxIter); A_best, B_best,
 * C_best, valHist, valHist1, best_iter and stop_reason may be NULL.  device = -1
 * runs on the device set as tritd_ncvx_masked_f64 does (the A rows of the best
 * iterate are shard-local, B and C replicated; every shard takes the same
 * decisions because the score sums are reduced with the fit sums). */
tritd_status tritd_ncvx_holdout_f64(const double* X, const uint8_t* observed, const uint8_t* holdout,
                                    int64_t n1, int64_t n2, int64_t n3, int32_t r, double rho,
                                    double lambda, double gamma_A, double epsilon, double p,
                                    double theta, int32_t maxIter, double tol, int32_t patience,
                                    int32_t val_norm, const double* A0, const double* B0,
                                    const double* C0, double* A, double* B, double* C, double* O,
                                    double* errHist, int32_t* iters, double* A_best, double* B_best,
                                    double* C_best, double* valHist, double* valHist1,
                                    int32_t* best_iter, int32_t* stop_reason, int32_t device);

typedef struct tritd_als_session tritd_als_session;
tritd_status tritd_als_session_create(tritd_als_session** out, int32_t device, const double* X,
                                      int64_t ldX, int64_t n1, int64_t n2, int64_t n3, int64_t i0,
                                      int64_t i1, int32_t r, const tritd_opts* opts,
                                      const double* A0, const double* B0, const double* C0,
                                      tritd_comm* comm, uint32_t flags, int32_t quiet);
/* tritd_als_session_create with a mask (see tritd_als_masked_f64).  observed
 * points at the mask byte of X(i0,0,0); consecutive (j,t) fibres are ldX BYTES
 * apart (the mask has the shape and leading dimension of X, one byte per
 * element).  It is a device pointer exactly when TRITD_SESSION_D_ON_DEVICE is
 * set.  observed == NULL: as tritd_als_session_create.  A mask with no true
 * entry in any shard is TRITD_ERR_ARG (with a communicator: on every rank
 * alike). */
tritd_status tritd_als_session_create_masked(tritd_als_session** out, int32_t device,
                                             const double* X, const uint8_t* observed, int64_t ldX,
                                             int64_t n1, int64_t n2, int64_t n3, int64_t i0,
                                             int64_t i1, int32_t r, const tritd_opts* opts,
                                             const double* A0, const double* B0, const double* C0,
                                             tritd_comm* comm, uint32_t flags, int32_t quiet);
/* Whether the session was created with a mask, and the number of observed
 * entries of its shard (all of them without a mask).  Either may be NULL. */
tritd_status tritd_als_session_mask_info(tritd_als_session* s, int32_t* masked,
                                         int64_t* observed_count);
/* tritd_als_session_create_masked with a holdout mask (tritd_als_holdout_f64):
 * holdout follows the conventions of observed (the mask byte of X(i0,0,0),
 * fibres ldX BYTES apart, a device pointer exactly when
 * TRITD_SESSION_D_ON_DEVICE is set); observed may be NULL (all true).  A run
 * after a patience stop is a no-op, like one after a stop of :20.
 * tritd_als_session_set_ncvx on such a session is TRITD_ERR_UNSUPPORTED: this
 * session scores inside the ALS fit kernel.  The nonconvex solver with a holdout
 * is created by tritd_als_session_create_ncvx_holdout. */
tritd_status tritd_als_session_create_holdout(tritd_als_session** out, int32_t device,
                                              const double* X, const uint8_t* observed,
                                              const uint8_t* holdout, int64_t ldX, int64_t n1,
                                              int64_t n2, int64_t n3, int64_t i0, int64_t i1,
                                              int32_t r, const tritd_opts* opts, int32_t patience,
                                              const double* A0, const double* B0, const double* C0,
                                              tritd_comm* comm, uint32_t flags, int32_t quiet);
/* tritd_als_session_create_holdout for the nonconvex solver
 * (tritd_ncvx_holdout_f64): the arguments of that creator, val_norm (2 or 1)
 * and the six positional parameters of test.m:1.  The solver is fixed at
 * creation (tritd_als_session_set_ncvx on it is TRITD_ERR_STATE);
 * opts->maxIter and opts->tol are the maxIter and tol of test.m.
 * tritd_als_session_get_best, _get_O, _holdout_info and _get_val work on it;
 * _get_val2 returns both histories.  A run after a stop of either kind is a
 * no-op.  With a communicator every rank creates the session with the same
 * patience, val_norm and parameters. */
tritd_status tritd_als_session_create_ncvx_holdout(
    tritd_als_session** out, int32_t device, const double* X, const uint8_t* observed,
    const uint8_t* holdout, int64_t ldX, int64_t n1, int64_t n2, int64_t n3, int64_t i0, int64_t i1,
    int32_t r, const tritd_opts* opts, int32_t patience, int32_t val_norm, double rho, double lambda,
    double gamma_A, double epsilon, double p, double theta, const double* A0, const double* B0,
    const double* C0, tritd_comm* comm, uint32_t flags, int32_t quiet);
/* valHist and valHist1 (as many entries as errHist has; capacity maxIter each),
 * best_iter (0 before the first iteration) and stop_reason of a session made by
 * tritd_als_session_create_ncvx_holdout.  Any may be NULL.  Synchronises. */
tritd_status tritd_als_session_get_val2(tritd_als_session* s, double* valHist, double* valHist1,
                                        int32_t* best_iter, int32_t* stop_reason);
/* ms per timed iteration (tritd_als_session_set_timing) in the score kernel, and
 * from the end of the fit kernel to the start of the A update (score,
 * reductions, running best, snapshot).  Synchronises.  These two are
 * TRITD_ERR_STATE on any other session. */
tritd_status tritd_als_session_holdout_ms(tritd_als_session* s, double* score_ms, double* tail_ms);
/* The held-out entries (H & Omega) of the session's shard and
 * ||H .* Omega .* X|| over all shards.  Either may be NULL. */
tritd_status tritd_als_session_holdout_info(tritd_als_session* s, int64_t* count, double* norm);
/* valHist (as many entries as errHist has; capacity maxIter), best_iter
 * (0 before the first iteration) and stop_reason.  Any may be NULL.
 * Synchronises. */
tritd_status tritd_als_session_get_val(tritd_als_session* s, double* valHist, int32_t* best_iter,
                                       int32_t* stop_reason);
/* The factors iteration best_iter started with, shaped like those of
 * tritd_als_session_get (A: the shard's rows).  Any may be NULL.  Synchronises.
 * These three are TRITD_ERR_STATE on a session without a holdout. */
tritd_status tritd_als_session_get_best(tritd_als_session* s, double* A, double* B, double* C);
/* Turn an ALS session, masked or not, into the nonconvex solver of
 * fast_robust_triple_tensor/test.m:1-73 (the positional parameters of :1): the
 * outlier chain :36-48 fused into the fit, ridge 1e-12 + reweighted shrink on A
 * (:49, :77-92), errHist / stop / progress line at the end of the iteration
 * (:62-68; the line is printed every iteration unless the session is quiet).  On
 * a masked session the semantics are those of tritd_ncvx_masked_f64.  Must come
 * before the first tritd_als_session_run (else, or a second time,
 * TRITD_ERR_STATE); rho == 0 is TRITD_ERR_ARG. */
tritd_status tritd_als_session_set_ncvx(tritd_als_session* s, double rho, double lambda,
                                        double gamma_A, double epsilon, double p, double theta);
/* O of the session's shard (host, column-major, rows [i0, i1), leading
 * dimension ldO >= i1 - i0): that of iteration k-1 when the stop test broke the
 * loop at k (test.m:67 comes before O = O_new, :71), else that of the last
 * iteration run; exactly 0 where unobserved.  Synchronises.  TRITD_ERR_STATE on
 * a session without tritd_als_session_set_ncvx. */
tritd_status tritd_als_session_get_O(tritd_als_session* s, double* O, int64_t ldO);
tritd_status tritd_als_session_run(tritd_als_session* s, int32_t iters);
tritd_status tritd_als_session_sync(tritd_als_session* s, int32_t* iters_done, int32_t* stopped);
tritd_status tritd_als_session_get(tritd_als_session* s, double* A, double* B, double* C,
                                   double* errHist, int32_t* iters);
/* timing: fit kernel (fused triple product + error + W) and mode-3 MTTKRP ms per launch */
tritd_status tritd_als_session_set_timing(tritd_als_session* s, int32_t enable);
tritd_status tritd_als_session_kernel_ms(tritd_als_session* s, double* fit_ms, double* mode3_ms,
                                         double* iteration_ms, int32_t* samples);
tritd_status tritd_als_session_flags(tritd_als_session* s, uint32_t* flags);
void tritd_als_session_destroy(tritd_als_session* s);
/* Single-GPU rehearsal of the sharded ALS (virtual shards, as above). */
tritd_status tritd_als_sharded_virtual_f64(const double* X, int64_t n1, int64_t n2, int64_t n3,
                                           int32_t r, const tritd_opts* opts, const double* A0,
                                           const double* B0, const double* C0, int32_t nshards,
                                           double* A, double* B, double* C, double* errHist,
                                           int32_t* iters, int32_t device);

/* ---------------------------------------------------------------------------
 * Primitives (host pointers).  Each replaces the named reference file.
 * ------------------------------------------------------------------------- */
/* Qi-model triple product X(i,j,t) = sum_{p,q,s} A(i,q,s) B(p,j,s) C(p,q,t)
 * (origin_triple_tensor/triple_product.m:8-19 as intended; equals
 * reshape(unfold(A,1)*buildF(B,C)) with origin_triple_tensor/buildF.m:2-6).
 * Host and device (stream) forms; r <= 16. */
tritd_status tritd_triple_product_qi_f64(const double* A, const double* B, const double* C,
                                         int64_t n1, int64_t n2, int64_t n3, int32_t r, double* X);
tritd_status tritd_dev_triple_product_qi_f64(const double* A, const double* B, const double* C,
                                             int64_t n1, int64_t n2, int64_t n3, int32_t r,
                                             double* X, void* stream);
/* triple_product.m:1-7: X = reshape(unfold(A,1)*buildF(B,C), n1,n2,n3). */
tritd_status tritd_triple_product_f64(const double* A, const double* B, const double* C, int64_t n1,
                                      int64_t n2, int64_t n3, int32_t r, double* X);
/* unfold.m:1-13: mode 1 reshape, mode 2 permute [2 1 3], mode 3 permute [3 1 2]. */
tritd_status tritd_unfold_f64(const double* X, int64_t n1, int64_t n2, int64_t n3, int32_t mode,
                              double* Xn);
/* soft_threshold.m:1-2: sign(X).*max(abs(X)-lam,0), n elements. */
tritd_status tritd_soft_threshold_f64(const double* X, int64_t n, double lam, double* Y);
/* buildF.m / buildG.m / buildH.m.  which = 'F' (P=B (r,n2,r), Q=C (r,r,n3)),
 * 'G' (P=A (n1,r,r), Q=C), 'H' (P=A, Q=B (r,n2,r)).  out: r^2 x (nP*nQ). */
tritd_status tritd_build_design_f64(char which, const double* P, const double* Q, int64_t nP,
                                    int64_t nQ, int32_t r, double* out);

/* Driver metrics.
 * evaluate(X, gt, mask) of traffic_triple_comparison.m:194-202 (identical in
 * video_triple_comparison.m): rmse = norm(X(mask) - gt(:)), nrmse = rmse /
 * norm(gt(:)).  X has n elements; mask is n bytes (MATLAB logical, nonzero =
 * true) or NULL for true(size(X)); gt holds m = nnz(mask) elements in
 * column-major order of the true positions (m = n without a mask) — a
 * mismatch fails like MATLAB's "Arrays have incompatible sizes" (gt is never
 * read past m).  The device variant takes a mask at any byte alignment.  */
tritd_status tritd_evaluate_f64(const double* X, int64_t n, const double* gt, int64_t m,
                                const uint8_t* mask, double* rmse, double* nrmse);
/* quality_ybz(imagery1, imagery2) (other_methods/Low-rank-.../quality_ybz.m:1-33):
 * mean over the nf frames (n1 x n2 each; trailing dims folded into nf) of
 * psnr_index = 10*log10(255^2/mse(x-y)) and ssim_index (Gaussian 11x11
 * window, sigma 1.5, K = [0.01 0.03], L = 255, 'valid' map; -Inf for frames
 * smaller than 11x11).  psnr_frames / ssim_frames (nf each) may be NULL.
 * Any nf (launched in batches of 65535 frames). */
tritd_status tritd_quality_f64(const double* X1, const double* X2, int64_t n1, int64_t n2,
                               int64_t nf, double* psnr, double* ssim, double* psnr_frames,
                               double* ssim_frames);
tritd_status tritd_dev_evaluate_f64(const double* X, int64_t n, const double* gt, int64_t m,
                                    const uint8_t* mask, double* rmse, double* nrmse, void* stream);
tritd_status tritd_dev_quality_f64(const double* X1, const double* X2, int64_t n1, int64_t n2,
                                   int64_t nf, double* psnr, double* ssim, double* psnr_frames,
                                   double* ssim_frames, void* stream);

/* Foreground detection: eval(origin, groundtruth, background, foreground) of
 * video_triple_comparison.m:316-371.  With F the foreground,
 * G the CDnet labels (uint8: 255 = motion, 170 = unknown) and thr the
 * threshold (the reference's is 50, :339):
 *   p = abs(F) > thr (strict; NaN false, +-Inf true; a single F is widened),
 *   g = (G == 255), m = (G == 170), and per frame t (:347-360)
 *   TP = #(p & (g|m)), FP = #(p & ~g), FN = #(~p & g), TN = #(~p & (~g|m)).
 * pred receives p as bytes 0/1; counts is int64[nf][4] in the order TP, FP,
 * FN, TN, exact.  gt NULL: no counts (counts is not touched); pred NULL: no
 * mask; both NULL is TRITD_ERR_ARG, and so is thr < 0 or NaN.  The graythresh
 * level of :335-336 is computed and never used by the reference; it is not
 * restated.
 *
 * Session forms (video_triple_comparison.m:316-371 on the session's own O):
 * F is the O that tritd_session_get / tritd_als_session_get_O would return at
 * that moment (0 before the first ADMM iteration), thresholded where the
 * session keeps it: an ADMM session forms each element from its resident D,
 * Y_L and T and never materialises, converts or downloads O.  gt and pred
 * point at the byte of element (i0, 0, 0) of column-major arrays whose fibres
 * are ldG / ldP bytes apart (both >= i1 - i0); bytes of pred outside the
 * shard's rows are not written.  counts (host memory, n3 x 4) holds the
 * shard's rows only: a caller with several shards adds them, as it does the
 * parts of tritd_session_rre_parts; nothing is reduced across ranks.  With
 * TRITD_FG_DEVICE in flags gt and pred are device pointers on the session's
 * device, else host pointers staged through device buffers.  The call waits
 * for the session stream and leaves the session's state untouched.  The ALS
 * form is TRITD_ERR_STATE on a session that is not nonconvex. */
enum { TRITD_FG_DEVICE = 1u }; /* gt and pred are device pointers on the session's device */
tritd_status tritd_session_foreground(tritd_session* s, double thr, const uint8_t* gt, int64_t ldG,
                                      uint8_t* pred, int64_t ldP, int64_t* counts, uint32_t flags);
tritd_status tritd_als_session_foreground(tritd_als_session* s, double thr, const uint8_t* gt,
                                          int64_t ldG, uint8_t* pred, int64_t ldP, int64_t* counts,
                                          uint32_t flags);
/* ms of the kernel of the last tritd_session_foreground (eval of
 * video_triple_comparison.m:316-371) made while tritd_session_set_timing was
 * on, from HIP events around its launch: the staging copies and the wait are
 * not in it.  0 before the first such call. */
tritd_status tritd_session_foreground_ms(tritd_session* s, double* kernel_ms);
/* eval of video_triple_comparison.m:316-371 on a column-major n1 x n2 x nf
 * tensor F (double or single) in host memory; gt and pred are n1*n2*nf bytes. */
tritd_status tritd_foreground_f64(const double* F, const uint8_t* gt, int64_t n1, int64_t n2,
                                  int64_t nf, double thr, uint8_t* pred, int64_t* counts);
tritd_status tritd_foreground_f32(const float* F, const uint8_t* gt, int64_t n1, int64_t n2,
                                  int64_t nf, double thr, uint8_t* pred, int64_t* counts);
/* The same (video_triple_comparison.m:316-371) on device pointers F, gt and
 * pred with leading dimensions (element (i,j,t) at i + ld*(j + n2*t), each ld
 * >= n1); counts is host memory and the call waits for the stream. */
tritd_status tritd_dev_foreground_f64(const double* F, int64_t ldF, const uint8_t* gt, int64_t ldG,
                                      int64_t n1, int64_t n2, int64_t nf, double thr, uint8_t* pred,
                                      int64_t ldP, int64_t* counts, void* stream);
tritd_status tritd_dev_foreground_f32(const float* F, int64_t ldF, const uint8_t* gt, int64_t ldG,
                                      int64_t n1, int64_t n2, int64_t nf, double thr, uint8_t* pred,
                                      int64_t ldP, int64_t* counts, void* stream);
/* The scores of video_triple_comparison.m:316-371 (:356-365) from per-frame
 * counts[nf][4]: total = the sums over frames (TP, FP, FN, TN), precision =
 * TP/(TP+FP), recall = TP/(TP+FN), f1 = 2PR/(P+R), pwc = 100 (FP+FN)/numel,
 * in double; 0/0 is NaN as in MATLAB.  Host arithmetic only (no device is
 * needed); total and each score pointer may be NULL. */
tritd_status tritd_foreground_scores(const int64_t* counts, int64_t nf, int64_t numel,
                                     int64_t total[4], double* precision, double* recall,
                                     double* f1, double* pwc);

/* The video driver's report from a session: what
 * video_triple_comparison.m:56,64-67 computes after the solve, from the
 * session's resident tensors.  Notation: X the original tensor of the shard
 * (double, column-major, fibres ldX apart), m the byte mask of missing entries
 * (nonzero = missing, laid out like X with fibres ldM bytes apart; NULL:
 * nothing is missing), L the triple product of the session's current factors
 * (:56), O what tritd_session_get / tritd_als_session_get_O would return at
 * that moment.  The call returns raw parts, as tritd_session_rre_parts does,
 * so that a caller with several shards adds them:
 *   sums[0] = sum_m (L-X)^2     sums[1] = sum_m X^2       evaluate(X_hat, gt, mask)   :64
 *   sums[2] = sum_~m (O-X)^2    sums[3] = sum_~m X^2      evaluate(O, gt_2, ~mask)    :65
 *   sums[4] = sum ((L+O)-X)^2   sums[5] = sum X^2         evaluate(X_hat+O, X, true)  :66
 *   frame_sq[t]   = sum_ij (L-X)^2 of frame t, t < n3     psnr_index's numerator      :67
 *   frame_ssim[t] = ssim_index(X(:,:,t), L(:,:,t))        quality_ybz                 :67
 * frame_ssim[t] is -Inf when a frame is smaller than the 11 x 11 window, as
 * tritd_quality_f64 gives.  The figures follow on the host (evaluate, :290-298):
 * rmse = sqrt(S0), nrmse = sqrt(S0)/sqrt(S1), likewise srmse/snrmse from S2, S3
 * and trmse/tnrmse from S4, S5 (0/0 = NaN, as MATLAB gives for an empty gt);
 * psnr = mean_t 10 log10(255^2 / (frame_sq[t]/(n1 n2))), ssim = mean_t
 * frame_ssim[t].  An ADMM session before its first iteration and an ALS
 * session that is not nonconvex have O = 0: then S2 = S3 and S4 = sum (L-X)^2.
 * A masked session has O = 0 at its unobserved entries.
 *
 * Every sum is a fixed-order tree (no floating-point atomics): two calls give
 * the same bits.  Padding is never read from X or m.  sums (6 doubles),
 * frame_sq and frame_ssim (n3 doubles each) are host memory; sums or frame_sq
 * may be NULL, not both; frame_ssim == NULL means no SSIM and no scratch, else
 * the pass also writes L into a scratch of (i1-i0) n2 n3 doubles.  With
 * TRITD_REPORT_DEVICE in flags X and missing are device pointers on the
 * session's device, else host pointers staged through device buffers.  The
 * call waits for the session stream and writes nothing of the session: a run
 * after it continues bit for bit.
 * Errors, each before the first HIP call and in this order: NULL session, NULL
 * X, ldX < i1-i0, ldM < i1-i0 with a mask, sums and frame_sq both NULL (all
 * TRITD_ERR_ARG); an fp32 session (TRITD_ERR_UNSUPPORTED); frame_ssim on a
 * session that does not hold all rows (i0 > 0 or i1 < n1: the window crosses
 * row shards; TRITD_ERR_ARG, the sums and frame_sq still work there).  A
 * failed scratch allocation is TRITD_ERR_NOMEM. */
enum { TRITD_REPORT_DEVICE = 1u }; /* X and missing are device pointers on the session's device */
tritd_status tritd_session_report(tritd_session* s, const double* X, int64_t ldX,
                                  const uint8_t* missing, int64_t ldM, double* sums,
                                  double* frame_sq, double* frame_ssim, uint32_t flags);
/* The same (video_triple_comparison.m:56,64-67) on an ALS session: O is that
 * of tritd_als_session_get_O (iteration k-1 after a stop) for a nonconvex
 * session and 0 otherwise. */
tritd_status tritd_als_session_report(tritd_als_session* s, const double* X, int64_t ldX,
                                      const uint8_t* missing, int64_t ldM, double* sums,
                                      double* frame_sq, double* frame_ssim, uint32_t flags);
/* ms of the kernels of the last tritd_session_report (the pass of
 * video_triple_comparison.m:56,64-67, its reduction and, with frame_ssim, the
 * SSIM kernels) made while tritd_session_set_timing was on, from HIP events
 * around them: the staging copies and the wait are not in it.  0 before the
 * first such call. */
tritd_status tritd_session_report_ms(tritd_session* s, double* kernel_ms);

/* Device-pointer variants (for device-resident callers and the bench). */
tritd_status tritd_dev_unfold_f64(const double* X, int64_t n1, int64_t n2, int64_t n3, int32_t mode,
                                  double* Xn, void* stream);
tritd_status tritd_dev_soft_threshold_f64(const double* X, int64_t n, double lam, double* Y,
                                          void* stream);
tritd_status tritd_dev_triple_product_f64(const double* A, const double* B, const double* C,
                                          int64_t n1, int64_t n2, int64_t n3, int32_t r, double* X,
                                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRITD_H */
