// Device-resident TriTD-ADMM session (one mode-1 shard on one GPU).
#pragma once

#include <rccl/rccl.h>

#include <functional>
#include <thread>
#include <vector>

#include "holdout.h"
#include "kernels.h"

namespace tritd {
class GroupAbort;
}

struct tritd_comm {
    ncclComm_t comm = nullptr;             // RCCL (tritd_comm_create; group_comms)
    tritd_allreduce_fn host_fn = nullptr;  // or a host transport (tritd_comm_create_host)
    void* host_user = nullptr;
    int nranks = 1, rank = 0, device = 0;
    // a shard of a device group driven by run_threaded: its non-blocking RCCL
    // communicator is used only through the group's abort protocol (group.h)
    tritd::GroupAbort* group = nullptr;
    bool active() const { return comm != nullptr || host_fn != nullptr || group != nullptr; }
};

namespace tritd {

// Host output buffers of a device-to-host copy: populate their pages in
// parallel first (MADV_HUGEPAGE, then MADV_POPULATE_WRITE on up to 16
// threads; content unchanged).
// A fresh array (numpy zeros, mxCreate*) is mapped lazily, and the copy into
// it then runs at the single-threaded page-fault rate (~16 GB/s measured
// against ~55 GB/s into populated memory).  No-op below 64 MB.
void populate_output(void* p, size_t bytes);
void populate_output_threads(void* p, size_t bytes, unsigned max_threads);

// The one-shot calls' outputs O and E (whole tensors in the caller's memory)
// faulted in on a background thread while the iterations run on the device:
// a D2H copy into pages that fault runs at 12.6 instead of 30 GB/s
// (profiles/round6/pcie_probe.txt), and populating them in get() took as long
// as the copies.  join() before Session::get(..., populated = true).
class OutputPrefault {
public:
    OutputPrefault(void* O, void* E, size_t bytes);
    ~OutputPrefault() { join(); }
    void join();

private:
    std::thread t_;
};

// In-place all-reduce (sum, or max) of `count` doubles over the comm's ranks,
// ordered on stream st: ncclAllReduce, or the host transport (drains st).
void comm_allreduce(tritd_comm* c, double* buf, int64_t count, bool max, hipStream_t st);

// Host-side layout conversions between the reference shapes and the device
// factor layout (common.h / DESIGN.md §3).
void pack_A(const Geom& g, const double* A, std::vector<double>& Ah, std::vector<double>& AhT);
void pack_B(const Geom& g, const double* B, std::vector<double>& Bh);
void pack_C(const Geom& g, const double* C, std::vector<double>& Ch, std::vector<double>& ChT);
void unpack_A(const Geom& g, const std::vector<double>& Ah, double* A);
void unpack_B(const Geom& g, const std::vector<double>& Bh, double* B);
void unpack_C(const Geom& g, const std::vector<double>& Ch, double* C);
// the n doubles of a device factor through unpack_A/B/C into out (null: nothing)
void download_factor(const Geom& g, const double* dev, size_t n,
                     void (*unpack)(const Geom&, const std::vector<double>&, double*), double* out);
// the initial factors through pack_A/B/C into a session's device factors
// (ChF: C^ in single as well, the fp32 path; null: none)
void upload_factors(const Geom& g, const double* A0, const double* B0, const double* C0, double* Ah,
                    double* AhT, double* Bh, double* Ch, double* ChT, float* ChF = nullptr);

// One factor update (update_A/B/C, :77-81,86-88,93-95): Y = M * Ginv and its
// Gram.  Session::upd(mode) fills it for A, B, C (modes 0, 1, 2).
struct Update {
    const double* M = nullptr;  // the right-hand side in double (M2, M3; M1 of the fp64 path)
    const float* Mf = nullptr;  // or in single (M1 of the fp32 path)
    int64_t rows = 0;
    double* Ginv = nullptr;  // the Ginv slot of its solve
    double* Y = nullptr;     // the factor
    double* YT = nullptr;    // its transposed copy, leading dimension ldT (null: none)
    int64_t ldT = 0;
    float* YF = nullptr;  // its copy in single (C^ of the fp32 path)
    double* G = nullptr;  // where Y^T Y goes (A^TA behind M2 in red1_, BtB_, CtC_)
    // the generic apply runs the pinv fallback itself (A only: Session::solve
    // says why; B and C get it behind the solve, on the solve's stream)
    bool fix = false;
};

// What a session is made from: the data of a whole tensor (i0 = 0, i1 = n1) or
// of one mode-1 shard [i0, i1), the initial factors, the masks and the
// TRITD_SESSION_* flags.  D points at row i0; with TRITD_SESSION_D_ON_DEVICE
// it and the masks are device addresses.
struct ShardInputs {
    const void* D = nullptr;  // double, or float with TRITD_SESSION_F32
    int64_t ld = 0;           // elements between the fibres of D (and of the masks)
    int64_t n1 = 0, n2 = 0, n3 = 0, i0 = 0, i1 = 0;
    int r = 0;
    const double *A0 = nullptr, *B0 = nullptr, *C0 = nullptr;
    const uint8_t* observed = nullptr;  // a byte mask laid out like D, TRITD_OBSERVED_NAN or null
    HoldoutSpec ho;
    uint32_t flags = 0;
    size_t es() const { return (flags & TRITD_SESSION_F32) ? sizeof(float) : sizeof(double); }
    // the view of rows [a, b) of a whole-tensor description
    ShardInputs shard(int64_t a, int64_t b) const {
        ShardInputs s = *this;
        s.D = static_cast<const char*>(D) + a * es();
        s.i0 = a;
        s.i1 = b;
        s.observed = obs_rows(observed, a);
        s.ho = ho.rows(a);
        return s;
    }
};

class Session {
   public:
    // shared_stream, defer_normD: a device group driven phase by phase from one
    // host thread (api.cpp) shares a stream and reduces normD itself
    Session(int device, const ShardInputs& in, const tritd_opts& o, tritd_comm* comm = nullptr,
            hipStream_t shared_stream = nullptr, bool defer_normD = false);
    ~Session();

    // Enqueue iterations (full collective schedule; used without a virtual group)
    void run(int iters);
    void sync(int* done, int* stopped);
    // TRITD_FLAG_* raised by the device so far (read at every sync)
    uint32_t flags() const { return flags_; }
    // O, E: double, or float for an fp32 session.  populated: the caller has
    // already faulted in the pages of whole-tensor O and E (OutputPrefault)
    void get(double* A, double* B, double* C, void* O, void* E, int64_t ldOE, double* errHist,
             int* iters, bool populated = false);
    // dX: device tensor of the session's data type
    void rre_parts(const void* dX, int64_t ldX, double* num, double* den);
    bool is_f32() const { return f32_; }
    void counters(int64_t* dense_tiles_total, int64_t* tiles_per_launch);
    void k5_profile(int* dense_streams, int* slot_accesses) const {
        // dense-E mode: E^(k), E^(k-1) read and E^(k+1) written densely, no slots
        *dense_streams = de_ ? 7 : (dy_ ? 4 : 6);  // (fp32: 6, Y_O stored)
        *slot_accesses = de_ ? 0 : (dy_ ? 3 : 2);
    }
    bool dense_e() const { return de_; }
    // opts.observed: whether the session has a mask, and the observed entries
    // of its shard
    void mask_info(int* masked, int64_t* observed_count) const {
        if (masked) *masked = masked_ ? 1 : 0;
        if (observed_count) *observed_count = masked_ ? obs_count_ : g_.n1l * g_.n2 * g_.n3;
    }
    // holdout= (tritd.h, tritd_admm_holdout_f64): the entries of
    // H & Omega are withheld from the fit, which is the masked ADMM with
    // observed = Omega & ~H, and scored after K5 of every iteration from T.
    bool holdout() const { return holdout_; }
    // held-out entries of the shard; ||H o Omega o D|| and sum |.| over all shards
    void holdout_info(int64_t* count, double* norm, double* sum1) const {
        val_.info(count, norm, sum1);
    }
    // valHist, valHist1 (as many entries as errHist), best_iter, stop_reason
    void get_val(double* valHist, double* valHist1, int* best_iter, int* stop_reason);
    // the factors after iteration best_iter (A0, B0, C0 before any run)
    void get_best(double* A, double* B, double* C);
    // ms per timed iteration (TRITD_TIMING_ALL) in the score kernel, and from
    // the end of K5 to the end of the iteration (score, reductions, finish, snapshot)
    void holdout_ms(double* score, double* tail) const { val_.holdout_ms(acc_n_, score, tail); }
    // eval of video_triple_comparison.m:316-371 on the O that get() would
    // return now: pred = abs(O) > thr as column-major bytes of
    // the shard (fibres ldP apart; null: none), counts[n3][4] = TP, FP, FN, TN
    // per frame against the labels gt (fibres ldG apart; null: none).
    // on_device: gt and pred are device pointers.  O is not materialised and
    // nothing of the session is written; waits for the stream.
    void foreground(double thr, const uint8_t* gt, int64_t ldG, uint8_t* pred, int64_t ldP,
                    int64_t* counts, bool on_device);
    // ms of the kernel of the last foreground() made with timing on (events
    // around its launch; 0 before the first)
    double foreground_ms() const { return fg_ms_; }
    // The video driver's figures (video_triple_comparison.m:56,64-67;
    // DESIGN.md §17) on the current factors and the O that get() would return
    // now: the raw sums, frame squares and SSIM frames of ReportCall
    // (kernels.h), over the shard's rows.  fp64 sessions.  Nothing of the
    // session is written (the Qi model refreshes its H operand, which every
    // iteration rebuilds before use, as rre_parts does); waits for the stream.
    void report(const ReportCall& c);
    // ms of the kernels of the last report() made with timing on (0 before the first)
    double report_ms() const { return rp_ms_; }
    // doubles of red3 reduced over the shards at creation (normD^2, the fit
    // count; holdout: + ||H o Omega o D||^2, the held-out count, sum |.|) and in
    // every iteration of the phase schedules (holdout: + the two score sums)
    int norm_count() const { return holdout_ ? 5 : 2; }
    int red3_count() const { return holdout_ ? 4 : 2; }
    void set_timing(int level);  // 0 off, TRITD_TIMING_ALL, TRITD_TIMING_K5
    void kernel_ms(double* k5, double* m3, double* it, int* samples);
    // per timed iteration (TRITD_TIMING_ALL, with a communicator): ms inside
    // the iteration's all-reduces (issue to completion on the session stream,
    // so it includes waiting for the slowest rank) and their count
    void comm_ms(double* allreduce_ms, int* per_iter);
    const std::vector<double>& probe_ms() const { return probe_ms_; }
    int probe_pick() const { return probe_pick_; }

    // --- phase interface (virtual shard groups drive these directly) ------
    // Returns false when iteration k is beyond maxIter (nothing enqueued).
    int next_iter();  // reserves the next iteration number (or 0)
    void phaseA(int k);  // M1, solve A, A^TA partial, M2 partial -> red1
    void phaseB(int k);  // solve B, B^TB, M3 partial -> red2
    void phaseC(int k);  // solve C, C^TC, K5, norm partial -> red3
    void phaseD(int k);  // errHist / stop test
    double* red1() { return red1_.p; }
    double* red2() { return red2_.p; }
    double* red3() { return red3_.p; }
    int64_t red1_count() const { return g_.n2 * g_.RP + (int64_t)g_.RP * g_.RP; }
    int64_t red2_count() const { return g_.n3p * g_.RP; }
    hipStream_t stream() const { return st_; }
    // normD support for groups: local sum of squares in red3[0]
    void set_normD_from_red3();
    void maybe_print(int k);
    const Geom& geom() const { return g_; }
    int device() const { return device_; }

   private:
    // a communicator whose all-reduces run (one process per GPU, a host
    // transport, or a shard of a device group)
    bool sharded() const { return comm_ && comm_->active(); }
    void allreduce(double* buf, int64_t count);
    // side-stream schedule: the Grams of B, C and the R x R solves run on a
    // side stream, each overlapped with the big kernel that precedes its
    // consumer; with a communicator the same order with its all-reduces
    void iterate_side(int k);
    // single stream, no events (default for the fp64 CP model at RP <= 64):
    // the solves of update_C and of the next update_A run in an extra
    // workgroup of K2 / K5 (sweep.h), solve B on the main stream; with a
    // communicator the same order with its three all-reduces
    void iterate_fused(int k);
    bool fused_ = false;
    // K5's norm-partial count (its workgroups; the fp32 rank-split K5 has more)
    int k5n() const { return f32_ ? k5_parts32(g_) : k5_grid(g_) * g_.tsplit; }
    // pairs in red1_'s norm-partial tail: the largest k5n() over the ranks
    // (shards of different heights launch different K5 grids, and every rank
    // must all-reduce the same count); set by agree_counts()
    int k5tail_ = 0;
    void agree_counts();
    // K5's norm partials of iteration pend_k_ wait for the next iteration:
    // on one GPU in k5part_ for the extra workgroup of its M1 / M2; with a
    // communicator in red1_'s tail for its first all-reduce (one all-reduce
    // fewer per iteration); flush_norms() (all-reduces and) finishes them alone
    bool norms_pending_ = false;
    int pend_k_ = 0;
    double* norm_parts() const { return sharded() ? red1_.p + red1_count() : k5part_.p; }
    int norm_pairs() const { return sharded() ? k5tail_ : k5n(); }
    void flush_norms();
    bool shov_ = false;
    void create_streams(hipStream_t shared_stream);
    void side_after_main(hipEvent_t e);
    void launch_k5_full(int k, bool fused_finish);
    void launch_k5_pending(int k, const SideSolve& side = SideSolve{});
    // [M2 | A^TA] of this shard: red1_, all-reduced between update_A and update_B
    double* m2() const { return red1_.p; }
    double* ata() const { return red1_.p + g_.n2 * g_.RP; }
    Update upd(int mode) const;
    void apply(const Update& u);
    bool small_ag(int64_t rows) const;
    bool apply_gram(const Update& u, bool defer = false);
    bool side_gram_ok() const;
    bool side_gram_bc_ok() const;
    bool gram_a_in_m2() const;
    // the applies take the generic kernel (launch_apply_gen): fp32, or RP > 64
    bool gen_apply() const { return f32_ || g_.RP > 64; }
    FinishArgs take_finish(bool after_allreduce);
    bool overlap_ = false;
    hipStream_t side_ = nullptr;
    hipEvent_t evAtA_ = nullptr, evBtB_ = nullptr, evCtC_ = nullptr;
    hipEvent_t evSA_ = nullptr, evSB_ = nullptr, evSC_ = nullptr;
    DBuf GinvA_, GinvB_, GinvC_;
    // candidate pools timed with K5's access pattern; `overlap` (the host
    // copy of D) runs while the probe kernels do
    double* probe_pool(size_t pool_bytes, size_t slot, size_t stagger,
                       std::function<void()> overlap);
    DBuf dstage_;  // column-major staging of a host D (creation only)
    std::vector<double> probe_ms_;  // probe time of each candidate pool (ms)
    int probe_pick_ = 0;
    IterScalars scalars(int k) const;
    IterScalars32 scalars32(int k) const;
    // data-type dispatch of the per-iteration kernels
    void do_m1();
    void do_m2();
    void do_m3();
    void do_m3_qi();
    // partial: where the fp64 K5 writes its norm partials (null: k5part_);
    // side: the solve that rides in its extra workgroup
    void launch_k5_any(int k, bool prologue, double* partial = nullptr,
                       const SideSolve& side = SideSolve{});
    bool f32_ = false;
    size_t es_ = sizeof(double);  // bytes per element of D, O, E, Y_L, Y_O, T, W, M1
    DBuf ChF_;                    // C^ in single (fp32 path)

    int device_;
    hipStream_t st_ = nullptr;
    bool own_stream_ = false;
    Geom g_;
    tritd_opts o_;
    tritd_comm* comm_;
    std::vector<double> mu_;  // mu_[k-1] = muL = muO of iteration k
    double normD_ = 0.0;
    int k_enq_ = 0;

    DBuf pool_;  // declared first: destroyed after the views into it
    DBuf D_, O_, E_, YL_, YO_, T_, Wk_;
    DBuf CE_;  // compact E slots (common.h)
    // opts.observed (fp64 only): the mask words (common.h: MK), read by K5's
    // masked form in every schedule and by the O fix-up; D is stored with its
    // unobserved entries zeroed, so normD and the prologue need no mask
    DBuf M_;
    bool masked_ = false;
    int64_t obs_count_ = 0;
    double obs_count_d_ = 0.0;  // (the count as red3_[1]: summed over the shards beside normD^2)
    const unsigned long long* mask_words() const {
        return masked_ ? reinterpret_cast<const unsigned long long*>(M_.p) : nullptr;
    }
    void pack_mask(const uint8_t* observed, int64_t ldD, bool on_device,
                   const uint8_t* holdout = nullptr);
    // holdout=: M_ holds the fit words Omega & ~H, hset_ the held-out set and
    // val_ the validation state (holdout.h).  red3_[2..3] carry the score sums
    // of an iteration.
    bool holdout_ = false;
    HoldoutSet hset_;
    BestIterate val_;
    // the end of a holdout iteration: score, norm reduction, finish, snapshot
    // (holdout_tail: the fused and side-stream schedules; the phase schedules
    // call holdout_score after K5 and holdout_finish as their phase D)
    void holdout_tail(int k);
    void holdout_score(double* sums);
    void holdout_finish(int k, const double* ss, const double* hs);
    // derived Y_O (k_admm.hip, fp64 default, TRITD_DY=0 disables): E^(k) lives
    // in compact buffer k % 2 (CE_, CE2_) and dense buffer k % 2 (E_, and the
    // pool slot of Y_O, which is not stored in this mode)
    bool dy_ = false;
    // dense-E mode of K5 (k_admm.hip DE): de_mode_ -1 automatic (switch once E
    // has turned dense: checked after iterations 8 and 24), 0 never, 1 from the
    // start (TRITD_DENSE_E); de_prev_* = the dense-tile count at the last check
    bool de_ = false;
    int de_mode_ = -1;
    int64_t de_prev_ = 0;
    int de_prev_k_ = 0;
    bool de_eligible() const { return dy_ && !f32_ && !qi_ && g_.RP <= 64; }
    void maybe_dense_e(int k);
    DBuf CE2_;
    double* ce_buf(int k) const { return (dy_ && (k & 1)) ? CE2_.p : CE_.p; }
    double* e_buf(int k) const { return (dy_ && (k & 1)) ? YO_.p : E_.p; }
    // A^ (and its transpose) by iteration parity: iteration k writes
    // AhB_[k&1], so the A of the last finished iteration survives a next
    // iteration that has already started (the speculative start of
    // iterate_fused with a communicator); Ah_/AhT_ are views of the current one
    DBuf AhB_[2], AhTB_[2];
    // Ah_/AhT_ are valid only while iterations are being enqueued: after a
    // run they point at the parity of the last ENQUEUED iteration, which after
    // a stop (or a speculative iteration of the comm schedule) holds a newer
    // or partial A.  Readers after run() use finished_ah().
    DBuf Ah_, AhT_, Bh_, Ch_, ChT_, M1_, BtB_, CtC_;
    void set_ah(int k);
    // A^ of the last finished iteration `done` (as returned by sync)
    const double* finished_ah(int done) const { return AhB_[done & 1].p; }
    // Qi model (opts.model = TRITD_MODEL_QI, k_qi.hip): H = the Qi mode-3 design
    // matrix by rows ij (K2/K5 Khatri-Rao operand), an all-ones RP x RP block
    // (the Hadamard factor of the solve and the B operand of the KR product),
    // and the design Grams of the three solves
    bool qi_ = false;
    DBuf H_, ones_, GqA_, GqB_, GqC_;
    // inv(design Gram + alpha I) of update_A (mode 0), _B (1), _C (2): its
    // operands as the side job of M2 / K2 / K5 carries them (gram: the update
    // whose Gram that side job forms first), and the solve as a launch on s
    SideSolve side_solve(int mode, const Update* gram = nullptr) const;
    void solve(int mode, hipStream_t s, const FinishArgs* fin = nullptr);
    DBuf red1_, red2_, red3_;
    DBuf k5part_, m3part_, sqpart_;
    DBuf errHist_, errL_, errO_;
    uint32_t flags_ = 0;
    bool probe_ = false;  // TRITD_SESSION_PROBE: time candidate pools at creation
    int* ctrl_ = nullptr;  // [0] stop, [1] k done, [2] pinv-tolerance flag, then DENSE_SLOTS u64 dense-E counters
    unsigned long long* dense_tiles() const {
        return reinterpret_cast<unsigned long long*>(ctrl_ + 4);
    }

    int timing_ = 0;
    double fg_ms_ = 0.0;
    double rp_ms_ = 0.0;
    // timing event `slot` of this iteration (null: not timed), and its record
    hipEvent_t ev_slot(int slot) const {
        return timing_ ? ev_[ev_.size() - EV_SLOTS + slot] : nullptr;
    }
    void mark(int slot);
    // per timed iteration: EV_SLOTS events — 0 start, 1/2 K2, 3/4 K5, 5 end,
    // then a (before, after) pair per all-reduce of the iteration
    static constexpr int EV_AR = 4;  // all-reduce pairs timed per iteration
    static constexpr int EV_HO = 6 + 2 * EV_AR;  // holdout: (before, after) the score kernel
    static constexpr int EV_SLOTS = EV_HO + 2;
    std::vector<hipEvent_t> ev_;
    std::vector<int> ev_iter_;
    int ar_in_iter_ = 0;  // all-reduces issued so far in the current iteration
    double acc_k5_ = 0, acc_m3_ = 0, acc_it_ = 0, acc_ar_ = 0;
    int acc_n_ = 0, ar_per_iter_ = 0;
    void harvest_timing();
};

}  // namespace tritd
