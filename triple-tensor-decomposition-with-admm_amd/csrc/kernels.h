// Kernel launchers (host side) for libtritd.  All launches are asynchronous
// on the given stream; every ADMM-loop kernel early-exits when *stop != 0 so
// that iterations enqueued past the stop test of triple_decomp_ADMM.m:63
// become no-ops without a host round trip.
#pragma once

#include <functional>

#include "common.h"

namespace tritd {

// Dense-E tile statistics: one atomic per wave into one of DENSE_SLOTS
// counters (summed on the host), not one per tile on a single counter.
constexpr int DENSE_SLOTS = 64;

struct DevState;  // solver.cpp

// ---- K5: fused ADMM update (k_admm.hip) ----------------------------------
// One R x R solve run by an extra workgroup (blockIdx 0) of K2 or K5
// (sweep.h: side_solve): Ginv = inv(P o Q + alpha I).  on = 0: none.
struct SideSolve {
    const double* P = nullptr;
    const double* Q = nullptr;
    double alpha = 0.0;
    double* Ginv = nullptr;
    int* flags = nullptr;
    int R = 0;
    int on = 0;
    // gram_rows > 0: the side workgroup first forms one operand itself,
    // gram_to = X^T X of the row-major [gram_rows][RP] factor gram_src, which
    // then stands for P (gram_which = 0) or Q (1): the fused single-GPU
    // schedule's Grams ride in the side job instead of a launch of their own
    const double* gram_src = nullptr;
    double* gram_to = nullptr;
    int64_t gram_rows = 0;
    int gram_which = 0;
    // 0: the Gram only, no solve (a sharded session's A^T A, formed beside
    // M2 for the all-reduce that follows it)
    int solve = 1;
};

// The reduction + stop test of one iteration's K5 norm pairs, run by an
// extra workgroup of the next iteration's M1 (single GPU: one launch less per
// iteration; finish.h)
struct FinishArgs {
    double* p = nullptr;  // n [sum resL^2, sum resO^2] pairs
    int n = 0;
    double normD = 0.0;
    int k = 0;
    double tol = 0.0;
    double* errHist = nullptr;
    double* errL = nullptr;
    double* errO = nullptr;
    int* ctrl = nullptr;
    int single = 0;
    int clear = 0;
    int on = 0;
};

struct K5Args {
    const double* D;
    double* O;
    double* E;   // dense E: only tiles whose compact slot overflowed (common.h)
    double* CE;  // compact E: one 32-double slot per tile
    double* YL;
    double* T;
    double* Wk;
    const double* Ah;
    const double* Bh;
    const double* Ch;
    const double* ChT;
    double* partial;  // [grid][2] sums of resL^2, resO^2
    int64_t n1p, n2, n3p, plane, tiles, ntt;
    IterScalars s;
    const int* stop;
    unsigned long long* dense_tiles;  // DENSE_SLOTS running counts of E tiles stored densely
    // derived-Y_O mode (dy): Y_O is not stored; K5 of iteration k+1 rebuilds
    // Y_O^(k) = Y_L^(k) - muO_k (E^(k) - E^(k-1)) from E^(k) (CE/E) and
    // E^(k-1) (CEp/Ep) and writes E^(k+1) over E^(k-1) (k_admm.hip)
    double* CEp;
    double* Ep;
    // Khatri-Rao operand source: kr(ij,k) = Ah[j*ahj + i*RP + k] * Bh[j*bhj + k].
    // CP (the executed model): ahj = 0, bhj = RP.  Qi model (opts.model='qi'):
    // Ah = H (k_qi.hip, rows j*n1p+i), ahj = n1p*RP, Bh = ones, bhj = 0.
    int64_t ahj, bhj;
    SideSolve side;  // RP <= 64, CP model: solve A of the next iteration
    int tsplit = 1;  // chunks of the t-walk (set by launch_k5: k5_tsplit)
    // mask words of opts.observed (common.h: MK), or null: K5 then runs its
    // masked instantiation (the prologue never does: D is zeroed where unobserved)
    const unsigned long long* M = nullptr;
};
int k5_grid(const Geom& g);
// chunks of the fp64 K5's t-walk (1 unless the problem has few ij-tiles); K5
// then runs k5_grid * k5_tsplit workgroups and W needs k5_tsplit sets
int k5_tsplit(const Geom& g);
int k5_parts32(const Geom& g);  // fp32 K5's norm-partial count (its workgroups)
// dense_e: E kept densely for every tile (no compact slots; dy only, RP <= 64)
void launch_k5(const Geom& g, const K5Args& a, bool prologue, hipStream_t st,
               bool dense_e = false);
// O_k = (D + invL_next*Y_L) - T_{k+1} (O is not stored by K5)
void launch_pool_probe(const Geom& g, double* D, double* YL, double* T, double* CE,
                       hipStream_t st);
void launch_ce_expand(const Geom& g, const double* CE, double* E, hipStream_t st);
// (M: the mask words or null; O = 0 at unobserved elements)
void launch_o_fixup(const Geom& g, const double* D, const double* YL, const double* T,
                    double invL_next, double* O, hipStream_t st,
                    const unsigned long long* M = nullptr);
// partial sums -> out[0..1] (fixed-order tree)
void launch_reduce_pairs(const double* partial, int n, double* out, const int* stop, hipStream_t st);
// both in one launch (single GPU: nothing to all-reduce in between)
// single: D is of class single, so errHist(k) = single(norm/normD + norm/normD)
// with the norms rounded to single (MATLAB class rules)
void launch_reduce_finish(double* partial, int n, double normD, int k, double tol,
                          double* errHist, double* errL, double* errO, int* ctrl, bool single,
                          hipStream_t st, bool clear = false);
// errHist bookkeeping + stop test (triple_decomp_ADMM.m:59,63)
void launch_finish(const double* ss, double normD, int k, double tol, double* errHist, double* errL,
                   double* errO, int* ctrl, bool single, hipStream_t st);

// ---- contractions and small linear algebra (k_contract.hip) ---------------
// fin.on: the previous iteration's norm reduction and stop test in an extra
// workgroup (finish.h)
void launch_m1(const Geom& g, const double* Wk, const double* Bh, double* M1, const int* stop,
               hipStream_t st, const FinishArgs& fin = FinishArgs{});
// side: update_B's R x R solve in an extra workgroup (RP <= 64)
void launch_m2(const Geom& g, const double* Wk, const double* AhT, double* M2, const int* stop,
               hipStream_t st, const SideSolve& side = SideSolve{});
int m3_split(const Geom& g);
int m3_parts(const Geom& g);  // partial slabs of n3p*RP written by K2
// kr(ij,k) = Ah[j*ahj + i*RP + k] * Bh[j*bhj + k] (K5Args::ahj; bhj < 0 means RP)
// side: an R x R solve in an extra workgroup of the CP kernel (RP <= 64)
void launch_m3(const Geom& g, const double* T, const double* Ah, const double* Bh, double* part,
               double* M3, const int* stop, hipStream_t st, int64_t ahj = 0, int64_t bhj = -1,
               const SideSolve& side = SideSolve{});
// G = X^T X over `rows` rows of a row-major [rows][RP] factor
void launch_gram(int RP, const double* X, int64_t rows, double* G, const int* stop, hipStream_t st,
                 bool side = false);
// Ginv buffers, one per Gram slot (pinv.h): [0, RP^2) the inverse, read by
// the apply; [RP^2, 2 RP^2) the Gram, saved by a solve whose pivot test came
// near pinv's cutoff; [2 RP^2, 3 RP^2) eigenvector scratch of the RP > 64
// fallback; the request word at ginv_req (a double: R = replace the inverse
// by pinv of the saved R x R Gram, 0 = none).
// Past the request word: RP pivots and RP/16 step words of the multi-workgroup
// solve (k_solve_mw, RP = 128 / 256; zero-initialised with the buffer).
__host__ __device__ inline int64_t ginv_req(int RP) { return 3 * (int64_t)RP * RP; }
__host__ __device__ inline int64_t ginv_piv(int RP) { return ginv_req(RP) + 8; }
__host__ __device__ inline int64_t ginv_sync(int RP) { return ginv_piv(RP) + RP; }
inline size_t ginv_count(int RP) { return (size_t)ginv_sync(RP) + 16; }
// Ginv = inv(P o Q + alpha I) on the leading R x R block (zero elsewhere),
// plus the pinv request of pinv.h.  flags is unused by the solves since the
// pinv fallback raises TRITD_FLAG_PINV_TOL itself (kept for the call shape).
// fin.on (RP <= 64): the same launch first runs the norm reduction + stop
// test of the previous iteration (finish.h) — a sharded session's finish and
// update_B's solve both follow the first all-reduce, one launch for the two.
void launch_solve(int RP, int R, const double* P, const double* Q, double alpha, double* Ginv,
                  int* flags, const int* stop, hipStream_t st, const FinishArgs* fin = nullptr);
// Y = M * Ginv ([rows][RP]); optional transposed copy YT[k*ldT + i].  A set
// request word makes every workgroup use pinv(saved Gram) instead (pinv.h);
// flags[0] is raised when that pinv drops a singular value.
// Y = M * Ginv and G = Y^T Y in one workgroup (small problems: apply_gram_small)
bool apply_gram_small(int RP, int64_t rows);
void launch_apply_gram(int RP, const double* M, int64_t rows, const double* Ginv, double* Y,
                       double* YT, int64_t ldT, double* G, const int* stop, int* flags,
                       hipStream_t st);
void launch_apply(int RP, const double* M, int64_t rows, const double* Ginv, double* Y, double* YT,
                  int64_t ldT, const int* stop, int* flags, hipStream_t st);
// ---- Qi model (opts.model='qi', k_qi.hip; origin_triple_tensor/build{F,G,H}.m) ----
// H[(j*n1p+i)*RP + p+r*q] = sum_s Ah(i, q+r*s) Bh(j, p+r*s)  (zero for k >= R)
void launch_qi_h(const Geom& g, int r, const double* Ah, const double* Bh, double* H,
                 const int* stop, hipStream_t st);
// M1(i, q+r*s) = sum_j sum_p W(ij, p+r*q) Bh(j, p+r*s)
void launch_m1_qi(const Geom& g, int r, const double* Wk, const double* Bh, double* M1,
                  const int* stop, hipStream_t st);
// M2(j, p+r*s) = sum_i sum_q W(ij, p+r*q) Ah(i, q+r*s)
void launch_m2_qi(const Geom& g, int r, const double* Wk, const double* AhT, double* M2,
                  const int* stop, hipStream_t st);
// F F' / G G' / H H' of the Qi design matrices from the factor Grams
// (mode 0: X=B^TB, Y=C^TC; 1: X=A^TA, Y=C^TC; 2: X=A^TA, Y=B^TB)
void launch_qi_gram(int RP, int r, int mode, const double* X, const double* Y, double* out,
                    const int* stop, hipStream_t st);
void launch_fill(double* x, int64_t n, double v, hipStream_t st);
// out = sum_p in[p] (fixed order), written back to every in[p]  (virtual shards)
void launch_vsum(double* const* bufs, int nbufs, int64_t count, hipStream_t st);

// ---- primitives (k_prims.hip) ---------------------------------------------
void launch_sumsq_padded(const Geom& g, const double* X, double* partial, int nblocks,
                         hipStream_t st);
int sumsq_blocks(const Geom& g);
// triple product of device factors (layout of common.h) into / against a
// strided tensor X(i,j,t) = X[i + ldj*j + ldt*t] of the shard's n1l x n2 x n3:
// mode 0 writes L; mode 1 writes RRE partials partial[2*b] = sum (L-X)^2,
// [2*b+1] = sum X^2 (traffic_triple_comparison.m:62-63,194-199)
int tp_grid(const Geom& g);
void launch_tp(const Geom& g, const double* Ah, const double* Bh, const double* ChT, double* Lout,
               const double* X, double* partial, int mode, int64_t ldj, int64_t ldt,
               hipStream_t st, int64_t ahj = 0, int64_t bhj = -1);
// reference-layout device factors A (n1,r,r), B (r,n2,r), C (r,r,n3) -> Ah, Bh, ChT
void launch_pack_factors(const Geom& g, const double* A, const double* B, const double* C,
                         double* Ah, double* Bh, double* ChT, hipStream_t st);
void launch_transpose_batched(const double* in, double* out, int64_t rows, int64_t cols,
                              int64_t batch, hipStream_t st);
// layout conversions of the big tensors: column-major shard (leading dim ld,
// n1l x n2 x n3) <-> tile-major (common.h)
void launch_to_tm(const Geom& g, const double* src, int64_t ld, double* dst, hipStream_t st);
void launch_from_tm(const Geom& g, const double* src, double* dst, int64_t ld, hipStream_t st);
// opts.observed: the caller's byte mask (column-major shard like D, fibres ld
// bytes apart, nonzero = observed) -> mask words M (common.h: MK); the
// unobserved elements of the tile-major D are zeroed and the observed entries
// of the shard (pads excluded) added to *count.
// obs = TRITD_OBSERVED_NAN (here and in the two packers below): no byte mask
// is read, the observed bit is !isnan of the element of D itself (ld then
// belongs to hold alone).
void launch_mask_pack(const Geom& g, const uint8_t* obs, int64_t ld, unsigned long long* M,
                      double* D, unsigned long long* count, hipStream_t st);
// holdout=: obs (or null: all observed) and hold are byte masks like obs above.
// Eight words per tile (MK_WORDS_HO): 0-3 the fit mask Omega & ~H, 4-7 H & Omega.
// D is zeroed where unobserved only (the held-out values stay); padding is
// fit-observed and never held out; count[0] += |Omega & ~H|, count[1] += |H & Omega|
void launch_mask_pack_holdout(const Geom& g, const uint8_t* obs, const uint8_t* hold, int64_t ld,
                              unsigned long long* M, double* D, unsigned long long* count,
                              hipStream_t st);
// launch_sumsq_padded over a holdout session's D and mask words: partial[2b] is
// that of the tensor with the held-out entries zeroed (bitwise: they add +0),
// partial[2b + 1] the sum of squares of the held-out entries
void launch_sumsq_holdout(const Geom& g, const double* X, const unsigned long long* M,
                          double* partial, int nblocks, hipStream_t st);
void launch_soft_threshold(const double* X, int64_t n, double lam, double* Y, hipStream_t st);

// ---- held-out validation of the masked ADMM (k_holdout.hip) ---
// Packing, pass 1: obs (or null: all observed) and hold, byte masks like those
// of launch_mask_pack -> per tile ordinal b the four fit words Omega & ~H at
// M + MK_WORDS b (launch_mask_pack's layout: K5 and the O fix-up read them
// unchanged), the four words of H & Omega at Hw + MK_WORDS b in the same bit
// layout, and cnt[b] = the tile's held-out count.  Padding is fit-observed and
// never held out.  *fit_count += |Omega & ~H| of the shard (pads excluded).
// D (tile-major) is read only when obs = TRITD_OBSERVED_NAN, and not written.
void launch_ho_pack_words(const Geom& g, const uint8_t* obs, const uint8_t* hold, int64_t ld,
                          const double* D, unsigned long long* M, unsigned long long* Hw,
                          unsigned* cnt, unsigned long long* fit_count, hipStream_t st);
// hoff[b] = sum of cnt[0..b), b = 0..ntiles (hoff[ntiles] = the held-out
// count): one workgroup, a fixed order, no atomics
void launch_ho_scan(const unsigned* cnt, int64_t ntiles, unsigned long long* hoff, hipStream_t st);
// Packing, pass 2: the held-out values of tile b, in the bit order of its H
// words (word 0..3, lane 0..63 within a word), to vals + hoff[b]; D (tile-major)
// is then zeroed wherever the fit word is clear, held-out entries included.
void launch_ho_pack_vals(const Geom& g, const unsigned long long* M, const unsigned long long* Hw,
                         const unsigned long long* hoff, double* D, double* vals, hipStream_t st);
// partial[2b] = sum x^2, partial[2b + 1] = sum |x| over the n compact values
// (ho_sum_blocks(n) pairs, a fixed traversal)
int ho_sum_blocks(int64_t n);
void launch_ho_valsum(const double* vals, int64_t n, double* partial, int nblocks, hipStream_t st);
// valHist's sums after K5 of an iteration: T (TX order) holds the model value
// at every entry outside the fit mask, so d = x - T at each held-out element;
// partial[2b] = sum d^2, partial[2b + 1] = sum |d| (ho_score_grid(g) pairs).
// A tile without a held-out element is skipped before any load of T.
int ho_score_grid(const Geom& g);
void launch_ho_score(const Geom& g, const double* T, const unsigned long long* Hw,
                     const unsigned long long* hoff, const double* vals, double* partial,
                     const int* stop, hipStream_t st);
// The finish of a holdout session (one thread): finish_body (finish.h) on the
// norm sums ss, then valHist(k) = sqrt(hs[0]) / Hnorm, valHist1(k) = hs[1] /
// Hsum1, the running best of the history val_norm picks (a strict <, k = 1
// always taken), the snapshot request, the patience test.  hctrl = {best_iter,
// snapshot request, stop_reason}; best[0] = the best score so far.  An
// iteration enqueued after a stop clears the request.
void launch_finish_ho(const double* ss, const double* hs, double normD, double Hnorm, double Hsum1,
                      int k, double tol, int patience, int val_norm, double* errHist, double* errL,
                      double* errO, double* valHist, double* valHist1, int* ctrl, int* hctrl,
                      double* best, hipStream_t st);
// The finish of a nonconvex holdout session, in two one-thread
// kernels.  mark, after the fit of iteration k and before its A update:
// valHist(k) = sqrt(hs[0]) / Hnorm, valHist1(k) = hs[1] / Hsum1, the running
// best and the snapshot request, as launch_finish_ho.  finish, after the
// updates (test.m:62-68): errHist(k), the stop test of :65, then the patience
// test.  ctrl, hctrl and best as above; an iteration enqueued after a stop
// clears the request and writes nothing.
void launch_ncvx_ho_mark(const double* hs, double Hnorm, double Hsum1, int k, int val_norm,
                         double* valHist, double* valHist1, const int* ctrl, int* hctrl,
                         double* best, hipStream_t st);
void launch_ncvx_ho_finish(const double* ss, double Xnorm, int k, double tol, int patience,
                           double* errHist, int* ctrl, int* hctrl, hipStream_t st);

void launch_design(char which, const double* P, const double* Q, int64_t nP, int64_t nQ, int r,
                   double* out, hipStream_t st);

// ---- ALS variant (k_als.hip; triple_decomp_ALS.m) --------------------------
struct AlsFitArgs {
    const double* X;   // tile-major data tensor
    double* Wk;        // W = X x3 C^ (planes of n1p*n2)
    const double* Ah;
    const double* Bh;
    const double* Ch;
    double* partial;   // [grid][2]: sum (X - Xhat)^2, 0
    int64_t n1p, n2, n3p, plane, tiles, ntt;
    const int* stop;
    // nonconvex variant (fast_robust_triple_tensor/test.m:35-48; ncvx != 0):
    // Y = ((X - O) + rho*(L + Lam/rho))/onep; O' = shrink((X - Y) + Gam/rho, tau);
    // Lam += rho*(L - Y); Gam += rho*((X - Y) - O'); partial = sum ((X - Y) - O')^2.
    // O is double-buffered (O_in of iteration k-1, O_out of k), tile-major.
    int ncvx;
    const double* O_in;
    double *O_out, *Lam, *Gam;
    double rho, tau, onep;
    // masked form (observed=; M != null, ncvx == 0): the mask words of
    // launch_mask_pack (common.h: MK) and the TX copy of X~ = where(Omega, X,
    // Xhat) the kernel writes for this iteration's K2; X holds Omega o X
    const unsigned long long* M;
    double* XT;
    // held-out form (holdout=; != 0 with M and without ncvx): M holds the
    // eight words per tile of launch_mask_pack_holdout, X keeps its value at
    // a held-out entry, and partial[2b + 1] = sum (X - Xhat)^2 over H & Omega
    int holdout;
};
int als_fit_grid(const Geom& g);
void launch_als_fit(const Geom& g, const AlsFitArgs& a, hipStream_t st);
void launch_als_finish(const double* ss, double Xnorm, int k, double tol, double* errHist,
                       int* ctrl, hipStream_t st);
// holdout sessions: errHist(k), valHist(k), the running best,
// the stop test of :20, then the patience test; hctrl = {best_iter, snapshot
// request, stop_reason}, best[0] = valHist(best_iter)
void launch_als_finish_holdout(const double* ss, double Xnorm, double Hnorm, int k, double tol,
                               int patience, double* errHist, double* valHist, int* ctrl,
                               int* hctrl, double* best, hipStream_t st);
// copies Ah, Bh, Ch (na, nb, nc doubles) when hctrl[1] is set
void launch_als_snapshot(const double* Ah, const double* Bh, const double* Ch, double* Ab,
                         double* Bb, double* Cb, int64_t na, int64_t nb, int64_t nc,
                         const int* hctrl, hipStream_t st);
void launch_tm_to_tx(const Geom& g, const double* src, double* dst, hipStream_t st);
// test.m:82-92: A1 <- sign(A1).*max(|A1| - gamma*(1./((|A1|+eps).^expo)), 0), into Ah and AhT
void launch_ncvx_shrink(const Geom& g, double* Ah, double* AhT, double gamma, double eps,
                        double expo, const int* stop, hipStream_t st);

// ---- driver-side metrics (k_metrics.hip) ------------------------------------
// evaluate (traffic_triple_comparison.m:194-202): out2 = {sum (X(mask)-gt)^2,
// sum gt^2}; mask may be null (X and gt paired elementwise, m == n); gt is
// read only below m (a mask with more true entries than m is reported by the
// caller through *total).  scratch_i64:
// evaluate_blocks(n) + 1 entries; part: 2*evaluate_blocks(n) doubles; *total
// receives nnz(mask) (untouched without a mask)
int64_t evaluate_blocks(int64_t n);
void launch_evaluate(const double* X, const double* gt, int64_t m, const uint8_t* mask, int64_t n,
                     int64_t* scratch_i64, double* part, double* out2, int64_t* total,
                     hipStream_t st);
// quality_ybz: per-frame psnr/ssim of n1 x n2 x nf tensors; win = the
// normalised 11x11 Gaussian (column-major, device); scratch: quality_scratch() doubles
size_t quality_scratch(int64_t n1, int64_t n2, int64_t nf);
void launch_quality(const double* X, const double* Y, int64_t n1, int64_t n2, int64_t nf,
                    const double* win, double C1, double C2, double* scratch, double* psnr,
                    double* ssim, hipStream_t st);

// ---- foreground detection (k_foreground.hip) ------------------
// eval of video_triple_comparison.m:316-371: pred = abs(F) > thr as bytes,
// counts[t][0..3] += TP, FP, FN, TN of frame t against the labels gt
// (255 = motion, 170 = unknown).  gt null: no counts; pred null: no mask.
// Where the tile-major form takes F from:
enum FgSource {
    FG_ADMM64 = 0,    // (D + invL_next Y_L) - T of an fp64 ADMM session (o_expr.h), 0 where M says unobserved
    FG_ADMM32 = 1,    // the same of an fp32 session, rounded to single
    FG_STORED64 = 2,  // a stored tile-major tensor, passed as D
    FG_ZERO = 3       // F = 0: nothing is read
};
struct FgArgs {
    const void* D = nullptr;
    const void* YL = nullptr;
    const void* T = nullptr;  // TX order
    double invL_next = 0.0;
    float invL_next32 = 0.0f;
    const unsigned long long* M = nullptr;  // mask words (common.h: MK) or null
    double thr = 0.0;
    // column-major bytes of the shard: element (i, j, t) at i + ld (j + n2 t)
    const uint8_t* gt = nullptr;
    int64_t ldG = 0;
    uint8_t* pred = nullptr;
    int64_t ldP = 0;
    unsigned long long* counts = nullptr;  // [n3][4], zero on entry
    // filled by the launcher from the geometry
    int64_t n1l = 0, n1p = 0, n2 = 0, n3 = 0, tiles = 0, ntt = 0;
    int vec = 0;
};
void launch_foreground_tm(const Geom& g, int src, const FgArgs& a, hipStream_t st);
// plain column-major F (double, or float when f32) of n1 x n2 x nf
void launch_foreground_cm(const void* F, bool f32, int64_t ldF, const uint8_t* gt, int64_t ldG,
                          uint8_t* pred, int64_t ldP, unsigned long long* counts, int64_t n1,
                          int64_t n2, int64_t nf, double thr, hipStream_t st);
// The host side of one call: a host gt (on_device = false) is staged into a
// device buffer of rows*cols bytes, the device counts are zeroed, `launch`
// runs with the device gt / pred / counts and their leading dimensions, then
// pred (rows bytes of each of the cols fibres) and counts[nf][4] return to the
// host and the stream is waited for.  kernel_ms (or null) receives the
// kernel's own time from events recorded around its launch.
void run_foreground(int64_t rows, int64_t cols, int64_t nf, const uint8_t* gt, int64_t ldG,
                    uint8_t* pred, int64_t ldP, int64_t* counts, bool on_device, hipStream_t st,
                    const std::function<void(const uint8_t*, int64_t, uint8_t*, int64_t,
                                             unsigned long long*)>& launch,
                    double* kernel_ms = nullptr);

// ---- the video driver's report from a session (k_report.hip) ----
// video_triple_comparison.m:56,64-67 in one pass over the shard: with L the
// triple product of the factors, O by RpSource, X the original and m the byte
// mask of missing entries (null: none),
//   sums[0..5] = sum_m (L-X)^2, sum_m X^2, sum_~m (O-X)^2, sum_~m X^2,
//                sum ((L+O)-X)^2, sum X^2
//   frame_sq[t] = sum_ij (L-X)^2 of frame t          (psnr_index's numerator)
// and, with Lout, L column-major (fibres n1l apart) for the SSIM kernels.
// Every sum is a fixed-order tree: two calls give the same bits.
enum RpSource {
    RP_ADMM64 = 0,    // (D + invL_next Y_L) - T of an fp64 ADMM session (o_expr.h), 0 where M says unobserved
    RP_STORED64 = 1,  // a stored tile-major tensor, passed as D
    RP_ZERO = 2       // O = 0: nothing is read
};
struct RpArgs {
    // the Khatri-Rao operands of launch_tp (ahj, bhj: its strides; bhj < 0: RP)
    const double* Ah = nullptr;
    const double* Bh = nullptr;
    const double* ChT = nullptr;
    int64_t ahj = 0, bhj = -1;
    const double* D = nullptr;
    const double* YL = nullptr;
    const double* T = nullptr;  // TX order
    double invL_next = 0.0;
    const unsigned long long* M = nullptr;  // mask words (common.h: MK) or null
    // column-major tensors of the shard: element (i, j, t) at i + ld (j + n2 t)
    const double* X = nullptr;
    int64_t ldX = 0;
    const uint8_t* missing = nullptr;
    int64_t ldM = 0;
    double* Lout = nullptr;
    // [grid][6] and [grid][n3] block partials (report_grid(g) workgroups)
    double* part = nullptr;
    double* fpart = nullptr;
    // filled by the launcher from the geometry
    int64_t n1l = 0, n1p = 0, n2 = 0, n3 = 0, n3p = 0, tiles = 0, ntt = 0;
};
int report_grid(const Geom& g);
// the pass and the reduction of its partials into sums6[6] and frame_sq[n3] (device)
void launch_report(const Geom& g, int src, const RpArgs& a, double* sums6, double* frame_sq,
                   hipStream_t st);
// One call's host side, shared by the two session classes.  X and missing are
// host pointers staged through device buffers, or (on_device) device pointers
// used where they lie; sums[6], frame_sq[n3], frame_ssim[n3] are host outputs
// (each may be null; frame_ssim null: no SSIM and no scratch; win: the 11 x 11
// window of ssim_index on the host, needed with frame_ssim).  Every device
// buffer is allocated before the first launch, so a failed allocation leaves
// nothing enqueued.  Waits for the stream.  kernel_ms (or null): the time of
// the kernels alone, from events around them.
struct ReportCall {
    const double* X = nullptr;
    int64_t ldX = 0;
    const uint8_t* missing = nullptr;
    int64_t ldM = 0;
    double* sums = nullptr;
    double* frame_sq = nullptr;
    double* frame_ssim = nullptr;
    const double* win = nullptr;
    bool on_device = false;
};
void run_report(const Geom& g, int src, RpArgs a, const ReportCall& c, hipStream_t st,
                double* kernel_ms);
// ssim_index of each frame alone (launch_quality without its PSNR half; the
// same kernels, so the same bits): scratch of ssim_scratch() doubles
size_t ssim_scratch(int64_t n1, int64_t n2, int64_t nf);
void launch_ssim(const double* X, const double* Y, int64_t n1, int64_t n2, int64_t nf,
                 const double* win, double C1, double C2, double* scratch, double* ssim,
                 hipStream_t st);

// ---------------------------------------------------------------------------
// fp32 data path (D of class single): T, O, E, Y_L, Y_O, W and
// the mode contractions in fp32; factors, Grams and solves in fp64.
// RP in {16, 32, 48, 64, 128, 256}.
// ---------------------------------------------------------------------------
struct IterScalars32 {
    float muL, muO, invL, invO, thr, den, invL_next;  // MATLAB: double scalar -> single
    float rden;  // 1/den in single (K5's division, k_admm32.hip)
};
struct K5Args32 {
    const float* D;
    float* O;
    float* E;   // dense E: only tiles whose compact slot overflowed
    float* CE;  // compact E: one 64-float slot per tile (k_admm32.hip)
    float* YL;
    float* YO;
    float* T;
    float* Wk;
    const double* Ah;
    const double* Bh;
    const float* ChF;  // C^ (n3p x RP) in single (the values are single-rounded already)
    double* partial;   // [grid][2] sums of resL^2, resO^2
    int64_t n1p, n2, n3p, plane, tiles, ntt;
    IterScalars32 s;
    const int* stop;
    unsigned long long* dense_tiles;
    int64_t slots;  // workgroups resident at once (2 per CU): the pair roles alternate per round
};
constexpr int CE32_SLOT = 64;  // floats per compact-E slot (50 values, their position bytes, the count)
bool rp_supported32(int RP);
int padded_rank32(int R);
void launch_k5_32(const Geom& g, const K5Args32& a, bool prologue, hipStream_t st);
void launch_to_tm32(const Geom& g, const float* src, int64_t ld, float* dst, hipStream_t st);
void launch_from_tm32(const Geom& g, const float* src, float* dst, int64_t ld, hipStream_t st);
void launch_sumsq32(const Geom& g, const float* X, double* partial, int nblocks, hipStream_t st);
void launch_o_fixup32(const Geom& g, const float* D, const float* YL, const float* T,
                      float invL_next, float* O, hipStream_t st);
void launch_ce_expand32(const Geom& g, const float* CE, float* E, hipStream_t st);
void launch_pool_probe32(const Geom& g, float* D, float* YL, float* YO, float* T, float* CE,
                         hipStream_t st);
void launch_widen(const float* x, int64_t n, double* y, hipStream_t st);
void launch_m1_32(const Geom& g, const float* Wk, const double* Bh, float* M1, const int* stop,
                  hipStream_t st);
void launch_m2_32(const Geom& g, const float* Wk, const double* AhT, double* M2, const int* stop,
                  hipStream_t st, const FinishArgs& fin = FinishArgs());
int m3_parts32(const Geom& g);
void launch_m3_32(const Geom& g, const float* T, const double* Ah, const double* Bh, double* part,
                  double* M3, const int* stop, hipStream_t st);
// Y = M * Ginv for any RP; M double or single (Mf); round32: results rounded to
// single (then stored as double; MATLAB's (X*F')*pinv(G) is single for single
// data); YT transposed copy, YF single copy (either may be null)
// (fix: the pinv fallback runs first, in k_pinv_fix: a one-workgroup launch
// that returns at once unless the request word is set; false when the caller
// launched it behind the solve already)
void launch_apply_gen(int RP, const double* M, const float* Mf, int64_t rows, double* Ginv,
                      double* Y, double* YT, int64_t ldT, float* YF, bool round32, const int* stop,
                      int* flags, hipStream_t st, bool fix = true);
// the pinv fallback alone (pinv.h): Ginv[0, RP^2) <- pinv(saved Gram) if requested
void launch_pinv_fix(int RP, double* Ginv, const int* stop, int* flags, hipStream_t st);

}  // namespace tritd
