// Held-out validation (holdout=, patience=, val_norm=), the
// host side both session classes share (solver.h, als.h): the arguments, the
// staging of the caller's byte masks, the compact held-out set of
// k_holdout.hip, and the validation state (histories, running best, best
// iterate, stop reason) with its readers.
#pragma once

#include "kernels.h"

namespace tritd {

// holdout: a byte mask laid out like the data (null: no holdout); patience >
// 0 stops at k when k - best_iter >= patience; val_norm in {2, 1} picks the
// history that decides (valHist or valHist1; ADMM and nonconvex sessions)
struct HoldoutSpec {
    const uint8_t* mask = nullptr;
    int patience = 0;
    int val_norm = 2;
    // the spec of the shard that starts at row i0 (as obs_rows)
    HoldoutSpec rows(int64_t i0) const { return {mask ? mask + i0 : nullptr, patience, val_norm}; }
};

// The observed / holdout byte masks of a shard where the packing kernels read
// them: device masks as they are, host masks staged as contiguous
// n1l x n2 x n3 byte arrays (copies ordered on st; the buffers live as long as
// this object).  TRITD_OBSERVED_NAN has no array and passes through.
struct StagedMasks {
    const uint8_t *obs, *hold;
    int64_t ld;
    StagedMasks(const Geom& g, const uint8_t* observed, const uint8_t* holdout, int64_t ld,
                bool on_device, hipStream_t st);

   private:
    DBuf sobs_, shold_;
};

// The refusals of a session's creation sums, reduced over the shards: ss =
// {norm^2, fit count, ||H o Omega o X||^2, held-out count}; name = the data
// array in the caller's words ("D", "X")
void check_creation_sums(const double* ss, bool masked, bool holdout, const char* name);

// The compact held-out set (k_holdout.hip): Hw the four words of H & Omega per
// tile, hoff the tiles' offsets into hvals, the held-out values in bit order.
class HoldoutSet {
   public:
    void alloc(const Geom& g);  // the score partials (every holdout shard, empty ones included)
    // obs, hold, ld: StagedMasks.  Writes the fit words Omega & ~H to M (MK_WORDS
    // per tile), moves the held-out values of the tile-major D into the set and
    // zeroes D outside the fit words; returns |Omega & ~H|.  Two host
    // synchronisations: the count sizes hvals, then the sums.
    int64_t pack(const Geom& g, const uint8_t* obs, const uint8_t* hold, int64_t ld, double* D,
                 unsigned long long* M, hipStream_t st);
    // out[0..1] = sum d^2, sum |d| over the shard's held-out entries, d = x - T
    // (T in TX order: the model value at every entry outside the fit mask);
    // before / after (or null) are recorded around the score kernel alone
    void score(const Geom& g, const double* T, double* out, const int* ctrl, hipStream_t st,
               hipEvent_t before = nullptr, hipEvent_t after = nullptr);
    int64_t count = 0;  // held-out entries of the shard
    // creation: sum x^2 over them, the count, sum |x| (a fixed order); a member,
    // so that an asynchronous copy to the device may read it
    double sums[3] = {0.0, 0.0, 0.0};

   private:
    DBuf Hw_, hoff_, hvals_, hopart_;
};

// The validation state of a holdout session.  hctrl[0] best_iter, [1] the
// snapshot request of the current iteration, [2] stop_reason (0 none, 1 the
// convergence test, 2 patience); hbest[0] = the best score so far.  The finish
// kernels (finish.h: ho_update_best, ho_stop_reason) write them.
struct BestIterate {
    BestIterate() = default;
    BestIterate(const BestIterate&) = delete;
    BestIterate& operator=(const BestIterate&) = delete;
    ~BestIterate() {
        if (hctrl) hip_quiet(hipFree(hctrl));
    }
    // hist entries per history (l1: valHist1 as well), na / nb / nc doubles of
    // the packed factors; everything zeroed on st
    void alloc(size_t hist, bool l1, size_t na, size_t nb, size_t nc, const HoldoutSpec& spec,
               hipStream_t st);
    // best_iter = 0 until the first iteration: the packed A0, B0, C0 (device)
    void seed(const double* Ah, const double* Bh, const double* Ch);
    // keeps Ah, Bh, Ch when the finish kernel just before asked for it
    void snapshot(const double* Ah, const double* Bh, const double* Ch, hipStream_t st);
    // after a sync that returned `done`; valHist1 only where the session keeps it
    void get_val(int done, double* vh, double* vh1, int* best_iter, int* stop_reason) const;
    void get_best(const Geom& g, double* A, double* B, double* C) const;
    void info(int64_t* cnt, double* norm, double* s1) const {
        if (cnt) *cnt = count;
        if (norm) *norm = Hnorm;
        if (s1) *s1 = Hsum1;
    }
    // ms per timed iteration (n of them) in the score kernel, and in the
    // iteration's whole validation tail
    void holdout_ms(int n, double* score, double* tail) const {
        if (score) *score = acc_score / (n ? n : 1);
        if (tail) *tail = acc_tail / (n ? n : 1);
    }
    int* hctrl = nullptr;
    DBuf hbest, valHist, valHist1, Abest, Bbest, Cbest;
    int patience = 0, val_norm = 2;
    int64_t count = 0;                // held-out entries of the shard
    double Hnorm = 0.0, Hsum1 = 0.0;  // ||H o Omega o X||, sum |H o Omega o X| over all shards
    double acc_score = 0.0, acc_tail = 0.0;
};

}  // namespace tritd
