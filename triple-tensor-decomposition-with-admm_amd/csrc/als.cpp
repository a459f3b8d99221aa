// Device-resident ALS loop of fast_robust_triple_tensor/triple_decomp_ALS.m:1-40.
//
// Iteration k (reference order):
//   fit    Xhat = triple_product(A,B,C), errHist(k) = ||X - Xhat||/Xnorm   :15-16
//          + W = X x3 C^ for the next two updates (k_als.hip)
//   print  every 5 iterations                                               :17-19
//   stop   k > 1 && |e_k - e_{k-1}| < tol e_{k-1}: truncate, return         :20-23
//          (device flag: the update kernels of k early-exit)
//   A      M1 = X1 F' from W, solve (B^TB o C^TC + 1e-9 I), apply          :25-28
//   B      M2 = X2 G' from W and the new A, solve (A^TA o C^TC + 1e-9 I)    :30-33
//   C      M3 = X3 H' (K2 over the TX copy of X), solve (A^TA o B^TB + 1e-9 I) :35-38
// Sharded along mode 1 like the ADMM: the fit sum, [M2 | A^TA]
// and M3 are the three reductions.
#include "als.h"

#include <cmath>
#include <cstdlib>

namespace tritd {

void emit_line(const char* line);  // api.cpp

// (the argument rules — patience, val_norm, rho — are api.cpp's: every
// construction passes them first)
AlsSession::AlsSession(int device, const ShardInputs& in, int maxIter, double tol,
                       const NcvxParams* ncvx, tritd_comm* comm, hipStream_t shared_stream,
                       bool defer_norm)
    : device_(device), maxIter_(maxIter < 0 ? 0 : maxIter), tol_(tol), comm_(comm) {
    if (ncvx && !in.ho.mask)
        throw Error(TRITD_ERR_ARG, "a nonconvex session without a holdout is made by enable_ncvx");
    try {  // (a constructor that throws runs no destructor: an all-false mask is refused here)
        init(in, ncvx, shared_stream, defer_norm);
    } catch (...) {
        release();
        throw;
    }
}

void AlsSession::init(const ShardInputs& in, const NcvxParams* ncvx, hipStream_t shared_stream,
                      bool defer_norm) {
    const double* X = static_cast<const double*>(in.D);
    const int64_t ldX = in.ld, n2 = in.n2, n3 = in.n3;
    const uint32_t flags = in.flags;
    const uint8_t *observed = in.observed, *holdout = in.ho.mask;
    TRITD_HIP(hipSetDevice(device_));
    g_ = make_geom(in.n1, n2, n3, in.i0, in.i1, in.r);
    hoscore_ = holdout && ncvx;
    if (!rp_supported(g_.RP))
        throw Error(TRITD_ERR_UNSUPPORTED, "r must be in 1..8 for the fp64 ALS path");
    if (shared_stream) {
        st_ = shared_stream;
    } else {
        own_stream_ = true;
        TRITD_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    }
    const size_t Np = (size_t)g_.Ntm;
    X_.alloc(Np);
    XT_.alloc(Np);
    TRITD_HIP(hipMemsetAsync(X_.p, 0, Np * sizeof(double), st_));
    Wk_.alloc((size_t)g_.RP * g_.plane);
    TRITD_HIP(hipMemsetAsync(Wk_.p, 0, Wk_.bytes(), st_));
    Ah_.alloc(g_.n1p * g_.RP);
    AhT_.alloc((size_t)g_.RP * g_.n1p);
    Bh_.alloc(g_.n2 * g_.RP);
    Ch_.alloc(g_.n3p * g_.RP);
    ChT_.alloc((size_t)g_.RP * g_.n3p);
    M1_.alloc(g_.n1p * g_.RP);
    // one inverse per Gram slot, kept across iterations (k_solve_ns refines
    // the previous one); zero = no start
    for (DBuf* b : {&GinvA_, &GinvB_, &GinvC_}) {
        b->alloc(ginv_count(g_.RP));  // inverse + pinv fallback space (pinv.h)
        TRITD_HIP(hipMemsetAsync(b->p, 0, b->bytes(), st_));
    }
    BtB_.alloc((size_t)g_.RP * g_.RP);
    CtC_.alloc((size_t)g_.RP * g_.RP);
    // 2 per iteration (4 on a nonconvex holdout session); 4 at the creation of
    // a holdout session (5 on a nonconvex one)
    red0_.alloc(6);
    red1_.alloc(red1_count());
    red2_.alloc(red2_count());
    fitpart_.alloc(2 * (size_t)als_fit_grid(g_));
    m3part_.alloc((size_t)m3_parts(g_) * g_.n3p * g_.RP);
    sqpart_.alloc(2 * (size_t)sumsq_blocks(g_));
    errHist_.alloc(maxIter_ > 0 ? (size_t)maxIter_ : 1);
    for (DBuf* b : {&errHist_, &red0_, &red1_, &red2_})
        TRITD_HIP(hipMemsetAsync(b->p, 0, b->n * sizeof(double), st_));
    TRITD_HIP(hipMalloc(&ctrl_, 4 * sizeof(int)));
    TRITD_HIP(hipMemsetAsync(ctrl_, 0, 4 * sizeof(int), st_));
    if (holdout) {
        holdout_ = true;
        val_.alloc(errHist_.n, /*l1=*/hoscore_, Ah_.n, Bh_.n, Ch_.n, in.ho, st_);
        if (hoscore_) hset_.alloc(g_);
    }

    // X -> tile-major, and its TX copy for the mode-3 contraction (one-off)
    if (g_.n1l > 0) {
        if (flags & TRITD_SESSION_D_ON_DEVICE) {
            launch_to_tm(g_, X, ldX, X_.p, st_);
        } else {
            DBuf tmp;
            tmp.alloc((size_t)(g_.n1l * n2 * n3));
            if (ldX == g_.n1l)  // contiguous: one 1-D copy (the 2-D form is slower from pageable memory)
                TRITD_HIP(hipMemcpyAsync(tmp.p, X, (size_t)(g_.n1l * n2 * n3) * sizeof(double),
                                         hipMemcpyHostToDevice, st_));
            else
                TRITD_HIP(hipMemcpy2DAsync(tmp.p, g_.n1l * sizeof(double), X, ldX * sizeof(double),
                                           g_.n1l * sizeof(double), (size_t)(n2 * n3),
                                           hipMemcpyHostToDevice, st_));
            launch_to_tm(g_, tmp.p, g_.n1l, X_.p, st_);
            TRITD_HIP(hipStreamSynchronize(st_));
        }
        // X <- Omega o X and the mask words (fill values, NaN included, never
        // enter: Xnorm below sees the zeroed X)
        if (observed || holdout)
            pack_mask(observed, ldX, (flags & TRITD_SESSION_D_ON_DEVICE) != 0, holdout);
    }
    // (a masked session's fit kernel writes the TX copy of the imputed
    // tensor in every iteration, before K2 reads it)
    if (!masked_) launch_tm_to_tx(g_, X_.p, XT_.p, st_);

    upload_factors(g_, in.A0, in.B0, in.C0, Ah_.p, AhT_.p, Bh_.p, Ch_.p, ChT_.p);
    if (holdout_) val_.seed(Ah_.p, Bh_.p, Ch_.p);

    // Xnorm = norm(X(:))  (:6)
    const int nb = sumsq_blocks(g_);
    if (hoscore_) {
        // X_ is zero outside the fit mask: the ordinary padded sum, which is how
        // Xnorm gets the bits of the masked call on Omega & ~H.
        // red0 = {Xnorm^2, |Omega & ~H|, ||H o Omega o X||^2, |H & Omega|, sum |H o Omega o X|}
        launch_sumsq_padded(g_, X_.p, sqpart_.p, nb, st_);
        launch_reduce_pairs(sqpart_.p, nb, red0_.p, nullptr, st_);
        const double c[4] = {(double)obs_count_, hset_.sums[0], hset_.sums[1], hset_.sums[2]};
        TRITD_HIP(hipMemcpyAsync(red0_.p + 1, c, sizeof c, hipMemcpyHostToDevice, st_));
        TRITD_HIP(hipStreamSynchronize(st_));
    } else if (holdout_) {
        // X_ holds the held-out values: the same traversal with +0 in their
        // place (bitwise the sum of the zeroed tensor), ||H o Omega o X||^2 beside it.
        // red0 = {Xnorm^2, |Omega & ~H|, ||H o Omega o X||^2, |H & Omega|}
        launch_sumsq_holdout(g_, X_.p, reinterpret_cast<const unsigned long long*>(M_.p), sqpart_.p,
                             nb, st_);
        launch_reduce_pairs(sqpart_.p, nb, red0_.p, nullptr, st_);
        const double c[2] = {(double)obs_count_, (double)val_.count};
        TRITD_HIP(hipMemcpyAsync(red0_.p + 2, red0_.p + 1, sizeof(double), hipMemcpyDeviceToDevice,
                                 st_));
        TRITD_HIP(hipMemcpyAsync(red0_.p + 1, &c[0], sizeof(double), hipMemcpyHostToDevice, st_));
        TRITD_HIP(hipMemcpyAsync(red0_.p + 3, &c[1], sizeof(double), hipMemcpyHostToDevice, st_));
        TRITD_HIP(hipStreamSynchronize(st_));
    } else {
        launch_sumsq_padded(g_, X_.p, sqpart_.p, nb, st_);
        launch_reduce_pairs(sqpart_.p, nb, red0_.p, nullptr, st_);
    }
    if (masked_ && !holdout_) {  // the observed count rides beside Xnorm^2 (summed over the shards)
        const double c = (double)obs_count_;
        TRITD_HIP(hipMemcpyAsync(red0_.p + 1, &c, sizeof(double), hipMemcpyHostToDevice, st_));
        TRITD_HIP(hipStreamSynchronize(st_));
    }
    if (!defer_norm) {
        allreduce(red0_.p, norm_count());
        set_norm_from_red0();
    }
    // Grams of the initial B, C (replicated)
    launch_gram(g_.RP, Bh_.p, g_.n2, BtB_.p, ctrl_, st_);
    launch_gram(g_.RP, Ch_.p, g_.n3p, CtC_.p, ctrl_, st_);
    TRITD_HIP(hipStreamSynchronize(st_));
    if (ncvx) start_ncvx(*ncvx);
}

void AlsSession::release() {
    hip_quiet(hipSetDevice(device_));
    if (st_) hip_quiet(hipStreamSynchronize(st_));
    for (auto e : ev_) hip_quiet(hipEventDestroy(e));
    ev_.clear();
    if (ctrl_) hip_quiet(hipFree(ctrl_));
    ctrl_ = nullptr;
    if (own_stream_ && st_) hip_quiet(hipStreamDestroy(st_));
    st_ = nullptr;
}

AlsSession::~AlsSession() { release(); }

void AlsSession::set_norm_from_red0() {
    double ss[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    TRITD_HIP(hipMemcpyAsync(ss, red0_.p, norm_count() * sizeof(double), hipMemcpyDeviceToHost, st_));
    TRITD_HIP(hipStreamSynchronize(st_));
    Xnorm_ = std::sqrt(ss[0]);
    check_creation_sums(ss, masked_, holdout_, "X");
    val_.Hnorm = std::sqrt(ss[2]);  // (zero without a holdout)
    val_.Hsum1 = ss[4];
}

// observed -> M_ (and X zeroed where unobserved), as Session::pack_mask.
// holdout (or null): a second byte mask of the same layout; the words are then
// those of launch_mask_pack_holdout and X keeps its held-out values.  The
// nonconvex holdout form packs like the ADMM: fit words
// Omega & ~H into M_, the held-out set into hset_, X_ zeroed outside the fit words.
void AlsSession::pack_mask(const uint8_t* observed, int64_t ldX, bool on_device,
                           const uint8_t* holdout) {
    masked_ = true;
    M_.alloc_bytes((size_t)(g_.Ntm / 256) * (holdout && !hoscore_ ? MK_WORDS_HO : MK_WORDS) *
                   sizeof(unsigned long long));
    const StagedMasks m(g_, observed, holdout, ldX, on_device, st_);
    unsigned long long* M = reinterpret_cast<unsigned long long*>(M_.p);
    if (hoscore_) {
        obs_count_ = hset_.pack(g_, m.obs, m.hold, m.ld, X_.p, M, st_);
        val_.count = hset_.count;
        return;
    }
    DBuf cnt;
    cnt.alloc(2);
    TRITD_HIP(hipMemsetAsync(cnt.p, 0, 2 * sizeof(double), st_));
    unsigned long long* dc = reinterpret_cast<unsigned long long*>(cnt.p);
    if (holdout)
        launch_mask_pack_holdout(g_, m.obs, m.hold, m.ld, M, X_.p, dc, st_);
    else
        launch_mask_pack(g_, m.obs, m.ld, M, X_.p, dc, st_);
    unsigned long long c[2] = {0, 0};
    TRITD_HIP(hipMemcpyAsync(c, cnt.p, sizeof c, hipMemcpyDeviceToHost, st_));
    TRITD_HIP(hipStreamSynchronize(st_));
    obs_count_ = (int64_t)c[0];
    val_.count = (int64_t)c[1];
}

void AlsSession::allreduce(double* buf, int64_t count) {
    if (!comm_ || !comm_->active()) return;
    comm_allreduce(comm_, buf, count, false, st_);
}

int AlsSession::next_iter() {
    if (k_enq_ >= maxIter_) return 0;
    return ++k_enq_;
}

void AlsSession::enable_ncvx(const NcvxParams& p) {
    if (k_enq_ > 0 || ncvx_)
        throw Error(TRITD_ERR_STATE, "the nonconvex solver is chosen once, before the first run");
    if (holdout_)
        throw Error(TRITD_ERR_UNSUPPORTED, "holdout is not supported by the nonconvex solver");
    p.check();
    start_ncvx(p);
}

void AlsSession::start_ncvx(const NcvxParams& p) {
    // (a masked session: the fit kernel runs the outlier chain on
    // X~ = where(Omega, X, T) and writes XT_ every iteration, as the masked ALS)
    TRITD_HIP(hipSetDevice(device_));
    ncvx_ = true;
    np_ = p;
    const size_t Np = (size_t)g_.Ntm;
    for (DBuf* b : {&Oa_, &Ob_, &Lam_, &Gam_}) {
        b->alloc(Np);
        TRITD_HIP(hipMemsetAsync(b->p, 0, Np * sizeof(double), st_));
    }
}

void AlsSession::phaseFit(int k) {
    AlsFitArgs a{};
    a.X = X_.p; a.Wk = Wk_.p; a.Ah = Ah_.p; a.Bh = Bh_.p; a.Ch = Ch_.p;
    a.partial = fitpart_.p;
    a.n1p = g_.n1p; a.n2 = g_.n2; a.n3p = g_.n3p; a.plane = g_.plane; a.tiles = g_.tiles;
    a.ntt = g_.ntt;
    a.stop = ctrl_;
    if (masked_) {  // X~ = where(Omega, X, Xhat) into XT_ for this iteration's K2
        a.M = reinterpret_cast<const unsigned long long*>(M_.p);
        a.XT = XT_.p;
        a.holdout = holdout_ && !hoscore_ ? 1 : 0;
    }
    if (ncvx_) {  // test.m:35-48; O of iteration k-1 in buffer (k-1)&1, O of k into k&1
        a.ncvx = 1;
        a.O_in = ((k - 1) & 1) ? Ob_.p : Oa_.p;
        a.O_out = (k & 1) ? Ob_.p : Oa_.p;
        a.Lam = Lam_.p;
        a.Gam = Gam_.p;
        a.rho = np_.rho;
        a.tau = np_.lambda / np_.rho;  // lambda/rho (:44); tau.*W_O = tau (W_O = ones, :43)
        a.onep = 1.0 + np_.rho;        // (1 + rho) (:36)
    }
    if (timing_) TRITD_HIP(hipEventRecord(ev_[ev_base_], st_));
    launch_als_fit(g_, a, st_);
    if (timing_) TRITD_HIP(hipEventRecord(ev_[ev_base_ + 1], st_));
    launch_reduce_pairs(fitpart_.p, als_fit_grid(g_), red0_.p, ctrl_, st_);
    if (hoscore_) {
        // XT_ holds T_k (:35) at every entry outside the fit mask; the two score
        // sums ride behind the fit sums in the same all-reduce
        hset_.score(g_, XT_.p, red0_.p + 2, ctrl_, st_, timing_ ? ev_[ev_base_ + 5] : nullptr,
                    timing_ ? ev_[ev_base_ + 6] : nullptr);
    }
}

void AlsSession::phaseErr(int k) {
    if (hoscore_) {
        // both scores and the running best; the factors iteration k started
        // with are kept, before the A update, if k is the best so far
        launch_ncvx_ho_mark(red0_.p + 2, val_.Hnorm, val_.Hsum1, k, val_.val_norm, val_.valHist.p,
                            val_.valHist1.p, ctrl_, val_.hctrl, val_.hbest.p, st_);
        val_.snapshot(Ah_.p, Bh_.p, Ch_.p, st_);
        if (timing_) TRITD_HIP(hipEventRecord(ev_[ev_base_ + 7], st_));
        return;
    }
    if (ncvx_) return;  // test.m takes errHist after the updates: phaseEnd
    if (holdout_) {
        // valHist(k), the running best and both stop tests; then the factors
        // iteration k started with are kept if k is the best so far
        launch_als_finish_holdout(red0_.p, Xnorm_, val_.Hnorm, k, tol_, val_.patience, errHist_.p,
                                  val_.valHist.p, ctrl_, val_.hctrl, val_.hbest.p, st_);
        val_.snapshot(Ah_.p, Bh_.p, Ch_.p, st_);
        return;
    }
    launch_als_finish(red0_.p, Xnorm_, k, tol_, errHist_.p, ctrl_, st_);
}

void AlsSession::phaseEnd(int k) {
    if (!ncvx_) return;
    // errHist(k) = norm(X(:) - Y_new(:) - O_new(:))/Xnorm (:62); the stop flag
    // set here makes every kernel of k+1 exit (:65-67)
    if (hoscore_) {  // + the patience test and stop_reason
        launch_ncvx_ho_finish(red0_.p, Xnorm_, k, tol_, val_.patience, errHist_.p, ctrl_, val_.hctrl,
                              st_);
        return;
    }
    launch_als_finish(red0_.p, Xnorm_, k, tol_, errHist_.p, ctrl_, st_);
}

void AlsSession::phaseA(int k) {
    (void)k;
    const int RP = g_.RP;
    double* M2 = red1_.p;
    double* AtA = red1_.p + g_.n2 * RP;
    launch_m1(g_, Wk_.p, Bh_.p, M1_.p, ctrl_, st_);
    // ALS :27 ridge 1e-9; test.m:82 ridge 1e-12, then the reweighted shrink :86-89
    launch_solve(RP, g_.R, BtB_.p, CtC_.p, ncvx_ ? 1e-12 : 1e-9, GinvA_.p, ctrl_ + 2, ctrl_, st_);
    launch_apply(RP, M1_.p, g_.n1p, GinvA_.p, Ah_.p, AhT_.p, g_.n1p, ctrl_, ctrl_ + 2, st_);
    if (ncvx_)
        launch_ncvx_shrink(g_, Ah_.p, AhT_.p, np_.gamma_A, np_.epsilon, np_.theta - np_.p, ctrl_,
                           st_);
    launch_gram(RP, Ah_.p, g_.n1p, AtA, ctrl_, st_);
    launch_m2(g_, Wk_.p, AhT_.p, M2, ctrl_, st_);
}

void AlsSession::phaseB(int k) {
    (void)k;
    const int RP = g_.RP;
    const double* M2 = red1_.p;
    const double* AtA = red1_.p + g_.n2 * RP;
    launch_solve(RP, g_.R, AtA, CtC_.p, 1e-9, GinvB_.p, ctrl_ + 2, ctrl_, st_);  // :32
    launch_apply(RP, M2, g_.n2, GinvB_.p, Bh_.p, nullptr, 0, ctrl_, ctrl_ + 2, st_);
    launch_gram(RP, Bh_.p, g_.n2, BtB_.p, ctrl_, st_);
    if (timing_) TRITD_HIP(hipEventRecord(ev_[ev_base_ + 2], st_));
    launch_m3(g_, XT_.p, Ah_.p, Bh_.p, m3part_.p, red2_.p, ctrl_, st_);
    if (timing_) TRITD_HIP(hipEventRecord(ev_[ev_base_ + 3], st_));
}

void AlsSession::phaseC(int k) {
    (void)k;
    const int RP = g_.RP;
    const double* AtA = red1_.p + g_.n2 * RP;
    launch_solve(RP, g_.R, AtA, BtB_.p, 1e-9, GinvC_.p, ctrl_ + 2, ctrl_, st_);  // :37
    launch_apply(RP, red2_.p, g_.n3p, GinvC_.p, Ch_.p, ChT_.p, g_.n3p, ctrl_, ctrl_ + 2, st_);
    launch_gram(RP, Ch_.p, g_.n3p, CtC_.p, ctrl_, st_);
}

void AlsSession::maybe_print(int k) {
    if (quiet_ || (!ncvx_ && k % 5 != 0)) return;  // ALS :17; test.m:63 prints every iteration
    if (comm_ && comm_->rank != 0) return;
    int ctrl[2];
    double e;
    TRITD_HIP(hipMemcpyAsync(ctrl, ctrl_, 2 * sizeof(int), hipMemcpyDeviceToHost, st_));
    TRITD_HIP(hipMemcpyAsync(&e, errHist_.p + (k - 1), sizeof(double), hipMemcpyDeviceToHost, st_));
    TRITD_HIP(hipStreamSynchronize(st_));
    if (ctrl[1] != k) return;  // the loop broke before iteration k
    char line[128];
    std::snprintf(line, sizeof line, "Iteration %d, relative error = %.4e", k, e);  // :18 (test.m:63)
    emit_line(line);
}

void AlsSession::run(int iters) {
    TRITD_HIP(hipSetDevice(device_));
    for (int it = 0; it < iters; ++it) {
        const int k = next_iter();
        if (!k) break;
        if (timing_) {
            ev_base_ = ev_.size();
            for (int e = 0; e < ev_slots(); ++e) {
                hipEvent_t ev;
                TRITD_HIP(hipEventCreate(&ev));
                ev_.push_back(ev);
            }
        }
        phaseFit(k);
        allreduce(red0_.p, fit_count());
        phaseErr(k);
        if (!ncvx_) maybe_print(k);
        phaseA(k);
        allreduce(red1_.p, red1_count());
        phaseB(k);
        allreduce(red2_.p, red2_count());
        phaseC(k);
        phaseEnd(k);
        if (ncvx_) maybe_print(k);
        if (timing_) TRITD_HIP(hipEventRecord(ev_[ev_base_ + 4], st_));
    }
}

void AlsSession::harvest_timing() {
    // events per iteration: [0] fit start, [1] fit end, [2] M3 start, [3] M3 end, [4] end
    // (nonconvex holdout: [5] score start, [6] score end, [7] snapshot end)
    const size_t ns = (size_t)ev_slots();
    for (size_t b = 0; b + ns <= ev_.size(); b += ns) {
        float it = 0, m3 = 0, fit = 0;
        TRITD_HIP(hipEventElapsedTime(&it, ev_[b], ev_[b + 4]));
        TRITD_HIP(hipEventElapsedTime(&fit, ev_[b], ev_[b + 1]));
        TRITD_HIP(hipEventElapsedTime(&m3, ev_[b + 2], ev_[b + 3]));
        acc_it_ += it;
        acc_fit_ += fit;
        acc_m3_ += m3;
        if (hoscore_) {
            float sc = 0, tl = 0;
            TRITD_HIP(hipEventElapsedTime(&sc, ev_[b + 5], ev_[b + 6]));
            TRITD_HIP(hipEventElapsedTime(&tl, ev_[b + 1], ev_[b + 7]));
            val_.acc_score += sc;
            val_.acc_tail += tl;
        }
        ++acc_n_;
    }
    for (auto e : ev_) hip_quiet(hipEventDestroy(e));
    ev_.clear();
}

void AlsSession::set_timing(bool on) {
    timing_ = on;
    acc_fit_ = acc_m3_ = acc_it_ = val_.acc_score = val_.acc_tail = 0;
    acc_n_ = 0;
}

void AlsSession::kernel_ms(double* fit, double* m3, double* it, int* samples) {
    const double n = acc_n_ ? (double)acc_n_ : 1.0;
    if (fit) *fit = acc_fit_ / n;
    if (m3) *m3 = acc_m3_ / n;
    if (it) *it = acc_it_ / n;
    if (samples) *samples = acc_n_;
}

void AlsSession::sync(int* done, int* stopped) {
    TRITD_HIP(hipSetDevice(device_));
    TRITD_HIP(hipStreamSynchronize(st_));
    if (!ev_.empty()) harvest_timing();
    int ctrl[3];
    TRITD_HIP(hipMemcpy(ctrl, ctrl_, 3 * sizeof(int), hipMemcpyDeviceToHost));
    if (ctrl[2] & 1) flags_ |= TRITD_FLAG_PINV_TOL;  // the pinv fallback dropped a value
    if (done) *done = ctrl[1];
    if (stopped) *stopped = ctrl[0];
}

void AlsSession::get(double* A, double* B, double* C, double* errHist, int* iters) {
    int done = 0, stopped = 0;
    sync(&done, &stopped);
    download_factor(g_, Ah_.p, Ah_.n, unpack_A, A);
    download_factor(g_, Bh_.p, Bh_.n, unpack_B, B);
    download_factor(g_, Ch_.p, Ch_.n, unpack_C, C);
    if (errHist && done > 0)
        TRITD_HIP(hipMemcpy(errHist, errHist_.p, (size_t)done * sizeof(double),
                            hipMemcpyDeviceToHost));
    if (iters) *iters = done;
}

void AlsSession::get_val(double* valHist, double* valHist1, int* best_iter, int* stop_reason) {
    int done = 0;
    sync(&done, nullptr);
    if (!holdout_) throw Error(TRITD_ERR_STATE, "get_val: not a holdout session");
    val_.get_val(done, valHist, valHist1, best_iter, stop_reason);
}

void AlsSession::get_best(double* A, double* B, double* C) {
    sync(nullptr, nullptr);
    if (!holdout_) throw Error(TRITD_ERR_STATE, "get_best: not a holdout session");
    val_.get_best(g_, A, B, C);
}

void AlsSession::get_O(double* O, int64_t ldO) {
    int done = 0, stopped = 0;
    sync(&done, &stopped);
    if (!ncvx_) throw Error(TRITD_ERR_STATE, "get_O: not a nonconvex (test.m) session");
    // :67 breaks before O = O_new (:71): a stop at k returns O of k-1
    const int kk = stopped ? done - 1 : done;
    const double* src = (kk & 1) ? Ob_.p : Oa_.p;  // kk = 0: the zero initial O
    if (g_.n1l > 0) {
        DBuf tmp;
        tmp.alloc((size_t)(g_.n1l * g_.n2 * g_.n3));
        launch_from_tm(g_, src, tmp.p, g_.n1l, st_);
        if (ldO == g_.n1l) {
            const size_t nb = (size_t)(g_.n1l * g_.n2 * g_.n3) * sizeof(double);
            populate_output(O, nb);
            TRITD_HIP(hipMemcpyAsync(O, tmp.p, nb, hipMemcpyDeviceToHost, st_));
        } else
            TRITD_HIP(hipMemcpy2DAsync(O, ldO * sizeof(double), tmp.p, g_.n1l * sizeof(double),
                                       g_.n1l * sizeof(double), (size_t)(g_.n2 * g_.n3),
                                       hipMemcpyDeviceToHost, st_));
        TRITD_HIP(hipStreamSynchronize(st_));
    }
}

void AlsSession::foreground(double thr, const uint8_t* gt, int64_t ldG, uint8_t* pred, int64_t ldP,
                            int64_t* counts, bool on_device) {
    int done = 0, stopped = 0;
    sync(&done, &stopped);
    if (!ncvx_) throw Error(TRITD_ERR_STATE, "foreground: not a nonconvex (test.m) session");
    const int kk = stopped ? done - 1 : done;  // the O of get_O
    FgArgs a;
    a.thr = thr;
    a.D = (kk & 1) ? Ob_.p : Oa_.p;
    run_foreground(g_.n1l, g_.n2 * g_.n3, g_.n3, gt, ldG, pred, ldP, counts, on_device, st_,
                   [&](const uint8_t* dg, int64_t ldg, uint8_t* dp, int64_t ldp,
                       unsigned long long* dc) {
                       a.gt = dg; a.ldG = ldg; a.pred = dp; a.ldP = ldp; a.counts = dc;
                       launch_foreground_tm(g_, FG_STORED64, a, st_);
                   });
}

void AlsSession::report(const ReportCall& c) {
    int done = 0, stopped = 0;
    sync(&done, &stopped);
    RpArgs a;
    a.Ah = Ah_.p; a.Bh = Bh_.p; a.ChT = ChT_.p;
    const int kk = stopped ? done - 1 : done;  // the O of get_O
    if (ncvx_) a.D = (kk & 1) ? Ob_.p : Oa_.p;
    run_report(g_, ncvx_ ? RP_STORED64 : RP_ZERO, a, c, st_, nullptr);
}

}  // namespace tritd
