// Device-resident ALS loop of fast_robust_triple_tensor/triple_decomp_ALS.m
// (SURVEY.md §8f rank 2): one mode-1 shard on one GPU, same factor layout
// and small kernels as the ADMM session (solver.h).
#pragma once

#include "solver.h"

namespace tritd {

// Parameters of the nonconvex solver of fast_robust_triple_tensor/test.m:1
// (positional in the reference: rho, lambda, gamma_A, epsilon, p, theta).
struct NcvxParams {
    double rho, lambda, gamma_A, epsilon, p, theta;
    // the one argument rule of the solver (test.m divides by rho)
    void check() const {
        if (!(rho != 0.0)) throw Error(TRITD_ERR_ARG, "rho must be non-zero");
    }
};

class AlsSession {
   public:
    // in.D: double, column-major shard rows [i0, i1) with leading dim in.ld
    // (host, or device with TRITD_SESSION_D_ON_DEVICE).  maxIter, tol: the only
    // opts fields the reference reads (triple_decomp_ALS.m:2-3).
    // in.observed (or null): the byte mask of the shard, laid out like X (fibres
    // ld bytes apart, nonzero = observed; host or device like X).  The
    // session then fits the observed entries only (tritd_als_masked_f64).
    // ncvx: with in.ho only (below); shared_stream, defer_norm as for Session.
    AlsSession(int device, const ShardInputs& in, int maxIter, double tol,
               const NcvxParams* ncvx = nullptr, tritd_comm* comm = nullptr,
               hipStream_t shared_stream = nullptr, bool defer_norm = false);
    ~AlsSession();
    AlsSession(const AlsSession&) = delete;
    AlsSession& operator=(const AlsSession&) = delete;

    void run(int iters);
    void sync(int* done, int* stopped);
    // TRITD_FLAG_* raised by the device so far (read at every sync)
    uint32_t flags() const { return flags_; }
    void get(double* A, double* B, double* C, double* errHist, int* iters);
    // the progress line of :17-19 (every 5 iterations, unconditional in the
    // reference); quiet = no host synchronisation for it (benchmarks)
    void set_quiet(bool q) { quiet_ = q; }
    void set_timing(bool on);
    void kernel_ms(double* fit, double* m3, double* it, int* samples);
    // Switch this session to the nonconvex solver of test.m (before run):
    // same fit/M1/M2/K2 kernels over X, plus the O / Lambda / Gamma ADMM
    // chain fused into the fit kernel, ridge 1e-12 + reweighted shrink on A,
    // errHist/stop/print at the END of the iteration (test.m:62-68).
    // After the first run (or a second time) it throws TRITD_ERR_STATE; rho = 0
    // is TRITD_ERR_ARG.  On a masked session the chain runs on
    // X~ = where(Omega, X, T): at an unobserved entry Y_new = T, O_new = 0,
    // Lambda and Gamma stay 0 and errHist gets nothing (tritd_ncvx_masked_f64).
    void enable_ncvx(const NcvxParams& p);
    bool ncvx() const { return ncvx_; }
    // whether the session has a mask, and the observed entries of its shard
    // (all of them without a mask)
    void mask_info(int* masked, int64_t* observed_count) const {
        if (masked) *masked = masked_ ? 1 : 0;
        if (observed_count) *observed_count = masked_ ? obs_count_ : g_.n1l * g_.n2 * g_.n3;
    }
    // ho.mask (or null; a byte mask like observed): the entries of H & Omega are
    // withheld from the fit, which is the masked ALS with observed = Omega & ~H,
    // and scored every iteration in the fit kernel's own pass:
    // valHist(k) = ||H o Omega o (X - Xhat)|| / ||H o Omega o X|| (tritd.h,
    // tritd_als_holdout_f64).  patience > 0 stops the loop at k when
    // k - best_iter >= patience.
    //
    // holdout with ncvx (the constructor's last argument):
    // the nonconvex solver of test.m with the same contract
    // (tritd_ncvx_holdout_f64).  The fit is the masked nonconvex one on
    // Omega & ~H, untouched; it leaves the model value of every held-out
    // entry in XT_, where k_ho_score (k_holdout.hip) reads it against a
    // compact copy of the held-out values.  Both scores are kept: valHist
    // (l2) and valHist1 (l1); val_norm in {2, 1} picks the one that decides.
    // The stop tests come after the updates (test.m:62-68).
    bool holdout() const { return holdout_; }
    bool ncvx_holdout() const { return hoscore_; }
    // held-out entries of the shard, ||H o Omega o X|| over all shards
    // (sum1: sum |H o Omega o X|, nonconvex holdout sessions only)
    void holdout_info(int64_t* count, double* norm, double* sum1 = nullptr) const {
        val_.info(count, norm, sum1);
    }
    // valHist(1:k), best_iter, stop_reason (0 none, 1 the test of :20, 2 patience)
    // valHist1: the l1 history of a nonconvex holdout session (else untouched)
    void get_val(double* valHist, double* valHist1, int* best_iter, int* stop_reason);
    // nonconvex holdout sessions, timed iterations: ms in the score kernel, and
    // from the end of the fit to the start of the A update (score, reductions,
    // mark, snapshot)
    void holdout_ms(double* score, double* tail) const { val_.holdout_ms(acc_n_, score, tail); }
    // the factors iteration best_iter started with (A0, B0, C0 before any run)
    void get_best(double* A, double* B, double* C);
    // doubles of the creation-time reduction: Xnorm^2, observed count
    // (holdout: + ||H o Omega o X||^2, held-out count; nonconvex holdout: + sum |H o Omega o X|)
    int norm_count() const { return hoscore_ ? 5 : (holdout_ ? 4 : 2); }
    // doubles of red0 reduced after the fit: the fit sums (nonconvex holdout:
    // + the two score sums)
    int fit_count() const { return hoscore_ ? 4 : 2; }
    // O returned by test.m: that of iteration k-1 when the stop test broke
    // the loop at k (:67 before :71), else the last one; column-major shard
    void get_O(double* O, int64_t ldO);
    // Session::foreground (solver.h) on the O of get_O, read where it is stored
    void foreground(double thr, const uint8_t* gt, int64_t ldG, uint8_t* pred, int64_t ldP,
                    int64_t* counts, bool on_device);
    // Session::report (solver.h) on the current factors and the O of get_O
    // (k - 1 after a stop); a session that is not nonconvex has O = 0
    void report(const ReportCall& c);

    // --- phase interface (device groups drive these; see api.cpp) -------
    int next_iter();
    void phaseFit(int k);  // fit kernel -> red0 (sum of squares)
    void phaseErr(int k);  // errHist(k), stop test
    void phaseA(int k);    // M1, solve A, apply A, A^TA partial, M2 partial -> red1
    void phaseB(int k);    // solve B, apply B, B^TB, M3 partial -> red2
    void phaseC(int k);    // solve C, apply C, C^TC
    void phaseEnd(int k);  // ncvx: errHist(k), stop test (after the updates, test.m:62-65)
    void maybe_print(int k);
    double* red0() { return red0_.p; }
    double* red1() { return red1_.p; }
    double* red2() { return red2_.p; }
    int64_t red1_count() const { return g_.n2 * g_.RP + (int64_t)g_.RP * g_.RP; }
    int64_t red2_count() const { return g_.n3p * g_.RP; }
    void set_norm_from_red0();
    hipStream_t stream() const { return st_; }
    int device() const { return device_; }
    const Geom& geom() const { return g_; }

   private:
    void allreduce(double* buf, int64_t count);
    int device_;
    hipStream_t st_ = nullptr;
    bool own_stream_ = false;
    Geom g_;
    int maxIter_;
    double tol_;
    tritd_comm* comm_;
    double Xnorm_ = 0.0;
    int k_enq_ = 0;
    bool quiet_ = false;
    DBuf X_, XT_, Wk_;  // X tile-major, X in TX order (K2), W = X x3 C^
    DBuf Ah_, AhT_, Bh_, Ch_, ChT_, M1_, GinvA_, GinvB_, GinvC_, BtB_, CtC_;
    DBuf red0_, red1_, red2_, fitpart_, m3part_, sqpart_, errHist_;
    uint32_t flags_ = 0;
    int* ctrl_ = nullptr;  // [0] stop, [1] errHist entries, [2] pinv-tolerance flag
    bool timing_ = false;
    std::vector<hipEvent_t> ev_;  // per timed iteration: ev_slots() events
    int ev_slots() const { return hoscore_ ? 8 : 5; }
    size_t ev_base_ = 0;  // first event of the iteration being enqueued
    double acc_fit_ = 0, acc_m3_ = 0, acc_it_ = 0;
    int acc_n_ = 0;
    void harvest_timing();
    bool ncvx_ = false;
    NcvxParams np_{};
    DBuf Oa_, Ob_, Lam_, Gam_;  // ncvx: O double buffer (iteration parity), duals (tile-major)
    // observed=: the mask words (common.h: MK) read by the masked fit kernel,
    // which also writes XT_ every iteration; X_ holds Omega o X, so Xnorm
    // needs no mask.  The observed count rides in red0_[1] at creation.
    DBuf M_;
    bool masked_ = false;
    int64_t obs_count_ = 0;
    void pack_mask(const uint8_t* observed, int64_t ldX, bool on_device,
                   const uint8_t* holdout = nullptr);
    // holdout=: M_ holds eight words per tile, X_ keeps the held-out values;
    // val_ is the validation state (holdout.h).
    bool holdout_ = false;
    BestIterate val_;
    // nonconvex holdout: M_ holds the four fit words per tile (Omega & ~H) the
    // masked nonconvex fit reads, X_ is zero outside them; the held-out set
    // lives in hset_ (holdout.h, the layout of k_holdout.hip).  The score sums
    // go to red0_[2..3] beside the fit sums.
    bool hoscore_ = false;
    HoldoutSet hset_;
    void start_ncvx(const NcvxParams& p);
    void init(const ShardInputs& in, const NcvxParams* ncvx, hipStream_t shared_stream,
              bool defer_norm);
    void release();  // what the destructor frees beyond the members' own
};

}  // namespace tritd
