// Held-out validation, the host side shared by Session and AlsSession (holdout.h).
#include "holdout.h"

#include "solver.h"

namespace tritd {

StagedMasks::StagedMasks(const Geom& g, const uint8_t* observed, const uint8_t* holdout,
                         int64_t ld0, bool on_device, hipStream_t st)
    : obs(observed), hold(holdout), ld(ld0) {
    if (on_device) return;
    const size_t rows = (size_t)(g.n2 * g.n3);
    auto to_device = [&](DBuf& b, const uint8_t* m) {
        b.alloc_bytes((size_t)g.n1l * rows);
        if (ld0 == g.n1l)
            TRITD_HIP(hipMemcpyAsync(b.p, m, (size_t)g.n1l * rows, hipMemcpyHostToDevice, st));
        else
            TRITD_HIP(hipMemcpy2DAsync(b.p, (size_t)g.n1l, m, (size_t)ld0, (size_t)g.n1l, rows,
                                       hipMemcpyHostToDevice, st));
        return reinterpret_cast<const uint8_t*>(b.p);
    };
    if (observed && !obs_is_nan(observed)) obs = to_device(sobs_, observed);
    if (holdout) hold = to_device(shold_, holdout);
    ld = g.n1l;
}

void check_creation_sums(const double* ss, bool masked, bool holdout, const char* name) {
    if ((masked || holdout) && ss[1] == 0.0)
        throw Error(TRITD_ERR_ARG, holdout ? "no observed entry is left to fit beside the holdout"
                                           : "observed has no true entry: nothing to fit");
    if (!holdout) return;
    if (ss[3] == 0.0) throw Error(TRITD_ERR_ARG, "holdout has no observed entry: nothing to score");
    if (ss[2] == 0.0)
        throw Error(TRITD_ERR_ARG, std::string("the held-out entries of ") + name + " are all zero");
}

void HoldoutSet::alloc(const Geom& g) { hopart_.alloc(2 * (size_t)ho_score_grid(g)); }

// words and per-tile counts, the offsets by a scan, then the compact values
// (their number is known only after the scan) and D zeroed outside the fit
// mask; the two sums of the values in a fixed order
int64_t HoldoutSet::pack(const Geom& g, const uint8_t* obs, const uint8_t* hold, int64_t ld,
                         double* D, unsigned long long* M, hipStream_t st) {
    const int64_t ntiles = g.Ntm / 256;
    DBuf cnt, tcnt, vpart, vsum;
    cnt.alloc(1);
    TRITD_HIP(hipMemsetAsync(cnt.p, 0, sizeof(double), st));
    Hw_.alloc_bytes((size_t)ntiles * MK_WORDS * sizeof(unsigned long long));
    hoff_.alloc((size_t)ntiles + 1);
    tcnt.alloc_bytes((size_t)ntiles * sizeof(unsigned));
    unsigned long long* Hw = reinterpret_cast<unsigned long long*>(Hw_.p);
    unsigned long long* hoff = reinterpret_cast<unsigned long long*>(hoff_.p);
    launch_ho_pack_words(g, obs, hold, ld, D, M, Hw, reinterpret_cast<unsigned*>(tcnt.p),
                         reinterpret_cast<unsigned long long*>(cnt.p), st);
    launch_ho_scan(reinterpret_cast<const unsigned*>(tcnt.p), ntiles, hoff, st);
    unsigned long long nh = 0, fit = 0;
    TRITD_HIP(hipMemcpyAsync(&nh, hoff + ntiles, sizeof nh, hipMemcpyDeviceToHost, st));
    TRITD_HIP(hipMemcpyAsync(&fit, cnt.p, sizeof fit, hipMemcpyDeviceToHost, st));
    TRITD_HIP(hipStreamSynchronize(st));
    count = (int64_t)nh;
    hvals_.alloc((size_t)nh);
    launch_ho_pack_vals(g, M, Hw, hoff, D, hvals_.p, st);
    const int nb = ho_sum_blocks(count);
    vpart.alloc(2 * (size_t)nb);
    vsum.alloc(2);
    launch_ho_valsum(hvals_.p, count, vpart.p, nb, st);
    launch_reduce_pairs(vpart.p, nb, vsum.p, nullptr, st);
    double hs[2] = {0.0, 0.0};
    TRITD_HIP(hipMemcpyAsync(hs, vsum.p, sizeof hs, hipMemcpyDeviceToHost, st));
    TRITD_HIP(hipStreamSynchronize(st));
    sums[0] = hs[0];
    sums[1] = (double)nh;
    sums[2] = hs[1];
    return (int64_t)fit;
}

void HoldoutSet::score(const Geom& g, const double* T, double* out, const int* ctrl,
                       hipStream_t st, hipEvent_t before, hipEvent_t after) {
    if (before) TRITD_HIP(hipEventRecord(before, st));
    launch_ho_score(g, T, reinterpret_cast<const unsigned long long*>(Hw_.p),
                    reinterpret_cast<const unsigned long long*>(hoff_.p), hvals_.p, hopart_.p, ctrl,
                    st);
    if (after) TRITD_HIP(hipEventRecord(after, st));
    launch_reduce_pairs(hopart_.p, ho_score_grid(g), out, ctrl, st);
}

void BestIterate::alloc(size_t hist, bool l1, size_t na, size_t nb, size_t nc,
                        const HoldoutSpec& spec, hipStream_t st) {
    patience = spec.patience;
    val_norm = spec.val_norm;
    valHist.alloc(hist);
    if (l1) valHist1.alloc(hist);
    hbest.alloc(1);
    Abest.alloc(na);
    Bbest.alloc(nb);
    Cbest.alloc(nc);
    for (DBuf* b : {&valHist, &valHist1, &hbest})
        if (b->p) TRITD_HIP(hipMemsetAsync(b->p, 0, b->bytes(), st));
    TRITD_HIP(hipMalloc(&hctrl, 4 * sizeof(int)));
    TRITD_HIP(hipMemsetAsync(hctrl, 0, 4 * sizeof(int), st));
}

void BestIterate::seed(const double* Ah, const double* Bh, const double* Ch) {
    TRITD_HIP(hipMemcpy(Abest.p, Ah, Abest.bytes(), hipMemcpyDeviceToDevice));
    TRITD_HIP(hipMemcpy(Bbest.p, Bh, Bbest.bytes(), hipMemcpyDeviceToDevice));
    TRITD_HIP(hipMemcpy(Cbest.p, Ch, Cbest.bytes(), hipMemcpyDeviceToDevice));
}

void BestIterate::snapshot(const double* Ah, const double* Bh, const double* Ch, hipStream_t st) {
    launch_als_snapshot(Ah, Bh, Ch, Abest.p, Bbest.p, Cbest.p, (int64_t)Abest.n, (int64_t)Bbest.n,
                        (int64_t)Cbest.n, hctrl, st);
}

void BestIterate::get_val(int done, double* vh, double* vh1, int* best_iter,
                          int* stop_reason) const {
    int h[3];
    TRITD_HIP(hipMemcpy(h, hctrl, sizeof h, hipMemcpyDeviceToHost));
    if (vh && done > 0)
        TRITD_HIP(hipMemcpy(vh, valHist.p, (size_t)done * sizeof(double), hipMemcpyDeviceToHost));
    if (vh1 && valHist1.p && done > 0)
        TRITD_HIP(hipMemcpy(vh1, valHist1.p, (size_t)done * sizeof(double), hipMemcpyDeviceToHost));
    if (best_iter) *best_iter = h[0];
    if (stop_reason) *stop_reason = h[2];
}

void BestIterate::get_best(const Geom& g, double* A, double* B, double* C) const {
    download_factor(g, Abest.p, Abest.n, unpack_A, A);
    download_factor(g, Bbest.p, Bbest.n, unpack_B, B);
    download_factor(g, Cbest.p, Cbest.n, unpack_C, C);
}

}  // namespace tritd
