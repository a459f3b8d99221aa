// Held-out validation of the masked ADMM (holdout=).
//
// The held-out entries H & Omega are withheld from the fit: the fit mask is
// Omega & ~H, and the masked K5 (k_admm.hip MK) leaves T_next = L exactly at
// every entry outside it.  So after K5 of iteration k the model value of every
// held-out entry sits in T, in TX order, and a streaming pass over T and a
// compact copy of the held-out values gives both scores.  K5 itself, K2, the
// prologue and the O fix-up are untouched.
//
// Per tile ordinal b (common.h): four fit words at M + 4 b (the layout of
// k_mask_pack), four words of H & Omega at Hw + 4 b in the same bit layout
// (bit l of word w = the element lane l holds in register w), and the tile's
// held-out values at vals + hoff[b], in the bit order of the H words (word
// 0..3, lane 0..63 within a word): the slot of a held-out element is the
// popcount of the H bits below it.  hoff is the exclusive prefix sum of the
// per-tile popcounts.
#include "finish.h"

namespace tritd {

typedef double d2v __attribute__((ext_vector_type(2)));

// NANM (TRITD_OBSERVED_NAN): the observed bit is !isnan of the
// lane's own element of the tile-major D (read only here: k_ho_pack_vals
// zeroes it afterwards), obs is not read.
template <bool NANM>
__global__ __launch_bounds__(256) void k_ho_pack_words(
    const uint8_t* __restrict__ obs, const uint8_t* __restrict__ hold, int64_t ld, int64_t n1l,
    int64_t n2, int64_t n3, int64_t n1p, int64_t ntt, int64_t ntiles,
    const double* __restrict__ D, unsigned long long* __restrict__ M,
    unsigned long long* __restrict__ Hw, unsigned* __restrict__ cnt, unsigned long long* fit_count) {
    const int l = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // tile ordinal
    if (blk >= ntiles) return;
    const int64_t q4 = blk >> 2, grp = q4 / ntt, tt = q4 - grp * ntt;
    const int64_t g = grp * 4 + (blk & 3);
    const int64_t row = 16 * g + (l & 15);
    const int64_t j = row / n1p, i = row - j * n1p;
    int fitn = 0, hon = 0;
#pragma unroll
    for (int w = 0; w < MK_WORDS; ++w) {
        const int64_t t = 16 * tt + (l >> 4) + 4 * w;
        const bool real = i < n1l && j < n2 && t < n3;
        const int64_t o = real ? (t * n2 + j) * ld + i : 0;
        bool on;
        if constexpr (NANM)
            on = !real || !is_nan_bits(D[(blk << 8) + ((w >> 1) << 7) + (l << 1) + (w & 1)]);
        else
            on = !real || !obs || obs[o] != 0;
        const bool ho = real && on && hold[o] != 0;  // a flag outside Omega is ignored
        const unsigned long long fw = __ballot(on && !ho), hw = __ballot(ho);
        fitn += __builtin_popcountll(__ballot(real && on && !ho));
        hon += __builtin_popcountll(hw);
        if (l == w) {
            M[blk * MK_WORDS + w] = fw;
            Hw[blk * MK_WORDS + w] = hw;
        }
    }
    if (l == 0) cnt[blk] = (unsigned)hon;
    if (l == 0 && fitn) atomicAdd(fit_count, (unsigned long long)fitn);
}

void launch_ho_pack_words(const Geom& g, const uint8_t* obs, const uint8_t* hold, int64_t ld,
                          const double* D, unsigned long long* M, unsigned long long* Hw,
                          unsigned* cnt, unsigned long long* fit_count, hipStream_t st) {
    const int64_t ntiles = g.Ntm / 256;
    const dim3 grid((unsigned)cdiv(ntiles, 4)), block(256);
    if (obs_is_nan(obs))
        hipLaunchKernelGGL(k_ho_pack_words<true>, grid, block, 0, st, nullptr, hold, ld, g.n1l, g.n2,
                           g.n3, g.n1p, g.ntt, ntiles, D, M, Hw, cnt, fit_count);
    else
        hipLaunchKernelGGL(k_ho_pack_words<false>, grid, block, 0, st, obs, hold, ld, g.n1l, g.n2,
                           g.n3, g.n1p, g.ntt, ntiles, D, M, Hw, cnt, fit_count);
    TRITD_CHECK_LAUNCH();
}

// One workgroup: thread t sums its contiguous run of tiles, thread 0 scans the
// 256 run sums, every thread then writes the offsets of its run.
__global__ __launch_bounds__(256) void k_ho_scan(const unsigned* __restrict__ cnt, int64_t n,
                                                 unsigned long long* __restrict__ hoff) {
    __shared__ unsigned long long s[256];
    const int t = threadIdx.x;
    const int64_t per = cdiv(n, 256);
    const int64_t b0 = (int64_t)t * per < n ? (int64_t)t * per : n;
    const int64_t b1 = b0 + per < n ? b0 + per : n;
    unsigned long long sum = 0;
    for (int64_t b = b0; b < b1; ++b) sum += cnt[b];
    s[t] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 0;
        for (int q = 0; q < 256; ++q) {
            const unsigned long long x = s[q];
            s[q] = run;
            run += x;
        }
    }
    __syncthreads();
    unsigned long long run = s[t];
    for (int64_t b = b0; b < b1; ++b) {
        hoff[b] = run;
        run += cnt[b];
    }
    if (t == 255) hoff[n] = run;  // (its run ends at n: the total)
}

void launch_ho_scan(const unsigned* cnt, int64_t ntiles, unsigned long long* hoff, hipStream_t st) {
    hipLaunchKernelGGL(k_ho_scan, dim3(1), dim3(256), 0, st, cnt, ntiles, hoff);
    TRITD_CHECK_LAUNCH();
}

__global__ __launch_bounds__(256) void k_ho_pack_vals(const unsigned long long* __restrict__ M,
                                                      const unsigned long long* __restrict__ Hw,
                                                      const unsigned long long* __restrict__ hoff,
                                                      int64_t ntiles, double* __restrict__ D,
                                                      double* __restrict__ vals) {
    const int l = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= ntiles) return;
    const unsigned long long base = hoff[blk];
    const unsigned long long below_lane = (1ull << l) - 1ull;
    int below = 0;
#pragma unroll
    for (int w = 0; w < MK_WORDS; ++w) {
        const unsigned long long hw = Hw[blk * MK_WORDS + w], fw = M[blk * MK_WORDS + w];
        const int64_t e = (blk << 8) + ((w >> 1) << 7) + (l << 1) + (w & 1);
        if ((hw >> l) & 1ull) vals[base + below + __builtin_popcountll(hw & below_lane)] = D[e];
        below += __builtin_popcountll(hw);
        if (!((fw >> l) & 1ull)) D[e] = 0.0;
    }
}

void launch_ho_pack_vals(const Geom& g, const unsigned long long* M, const unsigned long long* Hw,
                         const unsigned long long* hoff, double* D, double* vals, hipStream_t st) {
    const int64_t ntiles = g.Ntm / 256;
    hipLaunchKernelGGL(k_ho_pack_vals, dim3((unsigned)cdiv(ntiles, 4)), dim3(256), 0, st, M, Hw, hoff,
                       ntiles, D, vals);
    TRITD_CHECK_LAUNCH();
}

// lanes, then the four waves of the workgroup in order; thread 0 writes the pair
__device__ __forceinline__ void ho_block_pair(double a, double b, double* partial) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
    }
    __shared__ double ra[4], rb[4];
    if ((threadIdx.x & 63) == 0) {
        ra[threadIdx.x >> 6] = a;
        rb[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = ((ra[0] + ra[1]) + ra[2]) + ra[3];
        partial[2 * blockIdx.x + 1] = ((rb[0] + rb[1]) + rb[2]) + rb[3];
    }
}

__global__ __launch_bounds__(256) void k_ho_valsum(const double* __restrict__ vals, int64_t n,
                                                   double* partial) {
    double s = 0.0, a = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const double x = vals[e];
        s = fma(x, x, s);
        a += fabs(x);
    }
    ho_block_pair(s, a, partial);
}

int ho_sum_blocks(int64_t n) {
    const int64_t b = cdiv(n, 256 * 8);
    return (int)(b < 1024 ? (b < 1 ? 1 : b) : 1024);
}

void launch_ho_valsum(const double* vals, int64_t n, double* partial, int nblocks, hipStream_t st) {
    hipLaunchKernelGGL(k_ho_valsum, dim3(nblocks), dim3(256), 0, st, vals, n, partial);
    TRITD_CHECK_LAUNCH();
}

// One wave per tile, a workgroup's four waves walking tiles 4 blockIdx + wave,
// + 4 gridDim, ...  The tile's H words and offset are wave-uniform.  T is read
// in its own (TX) order as two contiguous 1 KB sweeps: lane l, slot s = 2h + q
// holds (i%16 = 4s + (l>>4), t%16 = l&15), which the mask words know as bit
// ((l&3) << 4) | (4s + (l>>4)) of word (l&15) >> 2 (common.h: TM register order).
__global__ __launch_bounds__(256) void k_ho_score(const double* __restrict__ T,
                                                  const unsigned long long* __restrict__ Hw,
                                                  const unsigned long long* __restrict__ hoff,
                                                  const double* __restrict__ vals, int64_t ntiles,
                                                  double* partial, const int* stop) {
    if (*stop) return;
    const int lane = threadIdx.x & 63;
    const int wsel = (lane & 15) >> 2;
    const int bit0 = ((lane & 3) << 4) | (lane >> 4);
    const d2v* T2 = reinterpret_cast<const d2v*>(T);
    double s2 = 0.0, s1 = 0.0;
    const int64_t step = (int64_t)gridDim.x * 4;
    // (wave-uniform: the words and the offset come through the scalar cache)
    auto uni = [](int64_t b) {
        return ((int64_t)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    };
    int64_t bu = uni((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    unsigned long long n0 = 0, n1 = 0, n2 = 0, n3 = 0, nbase = 0;
    if (bu < ntiles) {
        n0 = Hw[bu * MK_WORDS]; n1 = Hw[bu * MK_WORDS + 1];
        n2 = Hw[bu * MK_WORDS + 2]; n3 = Hw[bu * MK_WORDS + 3];
        nbase = hoff[bu];
    }
    for (; bu < ntiles; bu += step) {
        const unsigned long long h0 = n0, h1 = n1, h2 = n2, h3 = n3, base = nbase;
        // the next tile's words one step ahead, so that a tile costs one
        // round trip (its T and values) instead of two
        if (bu + step < ntiles) {
            const int64_t bn = bu + step;
            n0 = Hw[bn * MK_WORDS]; n1 = Hw[bn * MK_WORDS + 1];
            n2 = Hw[bn * MK_WORDS + 2]; n3 = Hw[bn * MK_WORDS + 3];
            nbase = hoff[bn];
        }
        if ((h0 | h1 | h2 | h3) == 0ull) continue;  // no held-out element: T is not read
        const int c0 = __builtin_popcountll(h0), c1 = __builtin_popcountll(h1),
                  c2 = __builtin_popcountll(h2);
        const unsigned long long hw = wsel == 0 ? h0 : (wsel == 1 ? h1 : (wsel == 2 ? h2 : h3));
        const int pre = (wsel > 0 ? c0 : 0) + (wsel > 1 ? c1 : 0) + (wsel > 2 ? c2 : 0);
        const d2v tv[2] = {T2[bu * 128 + lane], T2[bu * 128 + 64 + lane]};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int bit = bit0 + 4 * (2 * h + q);
                const bool held = (hw >> bit) & 1ull;
                double x = 0.0;
                if (held) x = vals[base + pre + __builtin_popcountll(hw & ((1ull << bit) - 1ull))];
                // a select, not a product: T may hold anything at the other elements
                const double d = held ? x - tv[h][q] : 0.0;
                s2 = fma(d, d, s2);
                s1 += fabs(d);
            }
    }
    ho_block_pair(s2, s1, partial);
}

int ho_score_grid(const Geom& g) {
    const int64_t b = cdiv(g.Ntm / 256, 4);
    return (int)(b < 2048 ? (b < 1 ? 1 : b) : 2048);
}

void launch_ho_score(const Geom& g, const double* T, const unsigned long long* Hw,
                     const unsigned long long* hoff, const double* vals, double* partial,
                     const int* stop, hipStream_t st) {
    hipLaunchKernelGGL(k_ho_score, dim3(ho_score_grid(g)), dim3(256), 0, st, T, Hw, hoff, vals,
                       g.Ntm / 256, partial, stop);
    TRITD_CHECK_LAUNCH();
}

__global__ void k_finish_ho(const double* ss, const double* hs, double normD, double Hnorm,
                            double Hsum1, int k, double tol, int patience, int val_norm,
                            double* errHist, double* errL, double* errO, double* valHist,
                            double* valHist1, int* ctrl, int* hctrl, double* best) {
    if (ctrl[0]) {
        hctrl[1] = 0;
        return;
    }
    finish_body(ss, normD, k, tol, errHist, errL, errO, ctrl, 0);  // :59-63
    const double v2 = sqrt(hs[0]) / Hnorm, v1 = hs[1] / Hsum1;
    valHist[k - 1] = v2;
    valHist1[k - 1] = v1;
    ho_update_best(val_norm == 1 ? v1 : v2, k, best, hctrl);
    ho_stop_reason(ctrl[0] != 0, k, patience, ctrl, hctrl);  // (:63 fired in finish_body)
}

void launch_finish_ho(const double* ss, const double* hs, double normD, double Hnorm, double Hsum1,
                      int k, double tol, int patience, int val_norm, double* errHist, double* errL,
                      double* errO, double* valHist, double* valHist1, int* ctrl, int* hctrl,
                      double* best, hipStream_t st) {
    hipLaunchKernelGGL(k_finish_ho, dim3(1), dim3(1), 0, st, ss, hs, normD, Hnorm, Hsum1, k, tol,
                       patience, val_norm, errHist, errL, errO, valHist, valHist1, ctrl, hctrl, best);
    TRITD_CHECK_LAUNCH();
}

// Held-out validation of the masked nonconvex solver.  The
// masked nonconvex fit stores x = fit ? X : T_k into its TX copy in every
// iteration, so k_ho_score reads that copy exactly as it reads the ADMM's T.
// The scores belong to the factors iteration k started with and are known
// after the fit; errHist(k) and the stop tests come after the updates
// (test.m:62-68).  So the finish is split in two one-thread kernels.
//
// After the fit of iteration k: both scores, the running best of the history
// val_norm picks (a strict <, k = 1 always taken), the snapshot request.
// hs = {sum d^2, sum |d|} over H & Omega, reduced over the shards.
__global__ void k_ncvx_ho_mark(const double* hs, double Hnorm, double Hsum1, int k, int val_norm,
                               double* valHist, double* valHist1, const int* ctrl, int* hctrl,
                               double* best) {
    if (ctrl[0]) {  // enqueued after a stop: nothing to keep
        hctrl[1] = 0;
        return;
    }
    const double v2 = sqrt(hs[0]) / Hnorm, v1 = hs[1] / Hsum1;
    valHist[k - 1] = v2;
    valHist1[k - 1] = v1;
    ho_update_best(val_norm == 1 ? v1 : v2, k, best, hctrl);
}

void launch_ncvx_ho_mark(const double* hs, double Hnorm, double Hsum1, int k, int val_norm,
                         double* valHist, double* valHist1, const int* ctrl, int* hctrl,
                         double* best, hipStream_t st) {
    hipLaunchKernelGGL(k_ncvx_ho_mark, dim3(1), dim3(1), 0, st, hs, Hnorm, Hsum1, k, val_norm,
                       valHist, valHist1, ctrl, hctrl, best);
    TRITD_CHECK_LAUNCH();
}

// After the updates of iteration k: errHist(k) (:62), the stop test of :65,
// then the patience test.  A stop of either kind leaves the updates of k in
// place, like the reference's break (O stays that of k-1, :71).
__global__ void k_ncvx_ho_finish(const double* ss, double Xnorm, int k, double tol, int patience,
                                 double* errHist, int* ctrl, int* hctrl) {
    if (ctrl[0]) return;
    const double e = sqrt(ss[0]) / Xnorm;
    errHist[k - 1] = e;
    ctrl[1] = k;
    ho_stop_reason(k > 1 && fabs(e - errHist[k - 2]) < tol * errHist[k - 2], k, patience, ctrl,
                   hctrl);
}

void launch_ncvx_ho_finish(const double* ss, double Xnorm, int k, double tol, int patience,
                           double* errHist, int* ctrl, int* hctrl, hipStream_t st) {
    hipLaunchKernelGGL(k_ncvx_ho_finish, dim3(1), dim3(1), 0, st, ss, Xnorm, k, tol, patience,
                       errHist, ctrl, hctrl);
    TRITD_CHECK_LAUNCH();
}

}  // namespace tritd
