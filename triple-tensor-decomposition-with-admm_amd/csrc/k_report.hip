// The video driver's report from a session: the eight figures
// video_triple_comparison.m:64-67 prints after the solve (:54) and
// X_hat = triple_product(A, B, C) (:56), from what the session holds.
//
//   evaluate(X_hat, X(m), m)          :64  S0 = sum_m (L-X)^2,    S1 = sum_m X^2
//   evaluate(O, X(~m), ~m)            :65  S2 = sum_~m (O-X)^2,   S3 = sum_~m X^2
//   evaluate(X_hat + O, X, true)      :66  S4 = sum ((L+O)-X)^2,  S5 = sum X^2
//   quality_ybz(X, X_hat)             :67  frame_sq[t] = sum_ij (L-X)^2 (psnr_index.m:4),
//                                          ssim_index(X(:,:,t), L(:,:,t))
// (evaluate: :290-298, rmse = norm(X(mask) - gt), nrmse = rmse / norm(gt).)
//
// k_report is k_tp<RP, 1> (k_prims.hip) with more to reduce: a wave owns one
// ij-tile, holds its Khatri-Rao row in registers and walks the t-tiles against
// the double-buffered C^T slice, RP/4 f64 MFMAs per tile.  The C/D fragment of
// L is the element order of the tile-major tensors (common.h), so the lane
// takes O for its four elements the way k_fg_tm does (two 16 B loads per
// tensor; T by element in TX order; the mask words), and X and the mask byte
// at the strided column-major position, as k_tp reads X.  All loads of a
// t-tile are issued before its MFMA chain.
//
// Reductions, all in a fixed order (no floating-point atomics): five sums stay
// in registers over the walk (the lane's sum of X^2 is its S1 + S3), then wave
// tree -> LDS -> part[block][6].
// The frame squares of a t-tile are summed over the 16 rows of the fragment
// (a 4-step xor tree inside each group of 16 lanes), over the workgroup's
// waves through LDS (double-buffered by t-tile parity, so the flush of tile
// tt - 1 shares the one barrier of tile tt), and leave as one partial per
// (workgroup, frame): fpart[block][t].  k_report_reduce then sums both over
// the workgroups.  Padding rows (i >= n1l), padded frames (t >= n3) and
// padding tiles are never read from X or m and never counted.
#include "kernels.h"
#include "o_expr.h"

namespace tritd {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2v __attribute__((ext_vector_type(2)));

constexpr int RPT_WAVES = 8;  // k_tp's workgroup (its measurements: k_prims.hip)

// Two workgroups per CU (128 VGPRs) where the Khatri-Rao row leaves room for
// it, RP <= 64: the pass is bound by its streams, and a second workgroup
// doubles the loads in flight.
template <int RP, int SRC>
__global__ __launch_bounds__(64 * RPT_WAVES, RP <= 64 ? 4 : 2) void k_report(RpArgs a) {
    constexpr int KS = RP / 4;
    constexpr int SK = 17;  // odd row stride of the [k][t] slice (k_tp)
    constexpr int NT = 64 * RPT_WAVES;
    constexpr int SP = RP * 8;
    constexpr int NS = (SP + NT - 1) / NT;
    __shared__ double sct[2][RP * SK];
    __shared__ double fsq[2][RPT_WAVES][16];
    __shared__ double red[6][RPT_WAVES];
    // the wave's number as a scalar: its tile, fibre and tile-major bases stay in SGPRs
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int il = lane & 15, tg = lane >> 4;
    const int64_t tile = (int64_t)blockIdx.x * RPT_WAVES + wid;
    const bool active = tile < a.tiles;
    const int64_t qper = a.n1p >> 4;
    const int64_t j = active ? tile / qper : 0;
    const int64_t i0 = active ? (tile - j * qper) << 4 : 0;
    const int64_t i = i0 + il;
    const bool row_ok = active && i < a.n1l;
    double kr[KS];
    if (KS <= 16) {
        // unconditional loads, all issued first (k_tp)
        double av[KS], bv[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + tg;
            av[s] = a.Ah[j * a.ahj + i * RP + k];  // kernels.h: KR source
            bv[s] = a.Bh[j * a.bhj + k];
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) kr[s] = active ? av[s] * bv[s] : 0.0;
    } else {
        // RP 128, 256: the row itself takes 64 / 128 registers, so the operands
        // are multiplied as they arrive
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = 4 * s + tg;
            const double p = a.Ah[j * a.ahj + i * RP + k] * a.Bh[j * a.bhj + k];
            kr[s] = active ? p : 0.0;
        }
    }
    const int64_t ntt = a.n3p >> 4;
    d2v sv[NS];
    auto stage_load = [&](int64_t tt) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int e = threadIdx.x + q * NT;
            if (SP % NT == 0 || e < SP) {
                const int k = e >> 3, t = (e & 7) * 2;
                sv[q] = *reinterpret_cast<const d2v*>(a.ChT + (int64_t)k * a.n3p + tt * 16 + t);
            }
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const int e = threadIdx.x + q * NT;
            if (SP % NT == 0 || e < SP) {
                const int k = e >> 3, t = (e & 7) * 2;
                sct[buf][k * SK + t] = sv[q][0];
                sct[buf][k * SK + t + 1] = sv[q][1];
            }
        }
    };
    // frame t of the t-tile tp: the waves' partials in wave order
    auto flush = [&](int64_t tp) {
        const int64_t t = tp * 16 + threadIdx.x;
        if (threadIdx.x < 16 && t < a.n3) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < RPT_WAVES; ++w) s += fsq[tp & 1][w][threadIdx.x];
            a.fpart[(int64_t)blockIdx.x * a.n3 + t] = s;
        }
    };
    // element (i, j, t = tb + 4r + tg): the lane's part of the offset (il, tg) is
    // loop-invariant, the rest is scalar
    const int64_t xt = a.ldX * a.n2, mt = a.ldM * a.n2, lt = a.n1l * a.n2;
    const int64_t xlane = il + xt * tg, mlane = il + mt * tg, llane = il + lt * tg;
    const int64_t xbase = i0 + a.ldX * j, mbase = i0 + a.ldM * j, lbase = i0 + a.n1l * j;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    stage_load(0);
    stage_store(0);
    __syncthreads();
#pragma unroll 1
    for (int64_t tt = 0; tt < ntt; ++tt) {
        const int buf = (int)(tt & 1);
        const bool more = tt + 1 < ntt;
        if (more) stage_load(tt + 1);
        // C/D element r of lane l: (i, j, t = 16 tt + (l>>4) + 4r), the tile-major
        // position (r>>1)*128 + 2l + (r&1) of tile (g = tile, tt)
        bool ok[4], miss[4];
        double x[4], o[4] = {0.0, 0.0, 0.0, 0.0};
        // (opaque: one scalar offset per t-tile instead of a running pointer per load)
        int64_t tb = tt * 16;
        asm volatile("" : "+s"(tb));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ok[r] = row_ok && tb + 4 * r + tg < a.n3;
            x[r] = ok[r] ? a.X[(xbase + xt * (tb + 4 * r)) + xlane] : 0.0;
            miss[r] = ok[r] && a.missing && a.missing[(mbase + mt * (tb + 4 * r)) + mlane] != 0;
        }
        if (SRC != RP_ZERO && active) {
            const int64_t base = tm_tile_base(tile, tt, ntt);
            const d2v d0 = *reinterpret_cast<const d2v*>(a.D + base + 2 * lane);
            const d2v d1 = *reinterpret_cast<const d2v*>(a.D + base + 128 + 2 * lane);
            o[0] = d0[0]; o[1] = d0[1]; o[2] = d1[0]; o[3] = d1[1];
            if (SRC == RP_ADMM64) {
                const d2v y0 = *reinterpret_cast<const d2v*>(a.YL + base + 2 * lane);
                const d2v y1 = *reinterpret_cast<const d2v*>(a.YL + base + 128 + 2 * lane);
                const double y[4] = {y0[0], y0[1], y1[0], y1[1]};
                // T: slot s = i>>2 of lane ((i&3)<<4)|t at (s>>1)*128 + 2 lane + (s&1) (k_o_fixup)
                const double* T = a.T + base;
                const int s = il >> 2;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int lx = ((il & 3) << 4) | (tg + 4 * r);
                    const double t = T[((s >> 1) << 7) + (lx << 1) + (s & 1)];
                    const bool obs = !a.M || ((a.M[((base >> 8) << 2) + r] >> lane) & 1ull);
                    o[r] = o_value(o[r], y[r], t, a.invL_next, obs);
                }
            }
        }
        const double* cT = sct[buf];
        d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < KS; ++s)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(cT[(4 * s + tg) * SK + il], kr[s], acc, 0, 0, 0);
        double fq[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double dl = acc[r] - x[r];
            const double dlq = dl * dl, xq = x[r] * x[r];
            const double dv = o[r] - x[r], dt = (acc[r] + o[r]) - x[r];
            fq[r] = ok[r] ? dlq : 0.0;
            s0 += miss[r] ? dlq : 0.0;
            s1 += miss[r] ? xq : 0.0;
            s2 += ok[r] && !miss[r] ? dv * dv : 0.0;
            s3 += ok[r] && !miss[r] ? xq : 0.0;
            s4 += ok[r] ? dt * dt : 0.0;
            if (a.Lout && ok[r])
                __builtin_nontemporal_store(acc[r], a.Lout + ((lbase + lt * (tb + 4 * r)) + llane));
        }
        // the 16 rows of the fragment, then lane il == 0 of each t-group files its four frames
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) fq[r] += __shfl_xor(fq[r], off);
        }
        if (il == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) fsq[buf][wid][tg + 4 * r] = fq[r];
        }
        if (tt > 0) flush(tt - 1);  // written before the barrier of tile tt - 1
        if (more) stage_store(buf ^ 1);  // buf^1 was last read in t-tile tt-1
        __syncthreads();
    }
    flush(ntt - 1);
    // every counted element is either missing or not: the lane's sum of X^2 is s1 + s3
    double sums[6] = {s0, s1, s2, s3, s4, s1 + s3};
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sums[q] += __shfl_xor(sums[q], off);
        if (lane == 0) red[q][wid] = sums[q];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < RPT_WAVES; ++w) s += red[threadIdx.x][w];
        a.part[(int64_t)blockIdx.x * 6 + threadIdx.x] = s;
    }
}

// part[grid][6] -> sums6 (the last workgroup), fpart[grid][n3] -> frame_sq
// (workgroup b: frames 16 b .. 16 b + 15), each a strided partial per thread
// and then a fixed-order sum: the same bits on every call.
__global__ __launch_bounds__(256) void k_report_reduce(const double* __restrict__ part,
                                                       const double* __restrict__ fpart,
                                                       int64_t grid, int64_t n3, double* sums6,
                                                       double* frame_sq) {
    __shared__ double sh[16][17];
    const int f = threadIdx.x & 15, q = threadIdx.x >> 4;
    double s = 0.0;
    if (blockIdx.x + 1 < gridDim.x) {
        const int64_t t = (int64_t)blockIdx.x * 16 + f;
        if (t < n3)
            for (int64_t b = q; b < grid; b += 16) s += fpart[b * n3 + t];
    } else if (f < 6) {
        for (int64_t b = q; b < grid; b += 16) s += part[b * 6 + f];
    }
    sh[q][f] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) v += sh[w][threadIdx.x];
        if (blockIdx.x + 1 < gridDim.x) {
            const int64_t t = (int64_t)blockIdx.x * 16 + threadIdx.x;
            if (t < n3) frame_sq[t] = v;
        } else if (threadIdx.x < 6) {
            sums6[threadIdx.x] = v;
        }
    }
}

int report_grid(const Geom& g) { return (int)cdiv(g.tiles, RPT_WAVES); }

void launch_report(const Geom& g, int src, const RpArgs& in, double* sums6, double* frame_sq,
                   hipStream_t st) {
    if (g.n3p % 16) throw Error(TRITD_ERR_ARG, "report: n3p must be a multiple of 16");
    if (cdiv(g.tiles, RPT_WAVES) > 0x7fffffffll)
        throw Error(TRITD_ERR_UNSUPPORTED, "report: shard too large");
    RpArgs a = in;
    if (a.bhj < 0) a.bhj = g.RP;
    a.n1l = g.n1l; a.n1p = g.n1p; a.n2 = g.n2; a.n3 = g.n3; a.n3p = g.n3p; a.tiles = g.tiles;
    a.ntt = g.ntt;
    const int nb = report_grid(g);
    const dim3 grid(nb), block(64 * RPT_WAVES);
#define RPT_SRC(RPV, S)                                                     \
    case S:                                                                 \
        hipLaunchKernelGGL((k_report<RPV, S>), grid, block, 0, st, a);      \
        break;
#define RPT_CASE(RPV)                  \
    case RPV:                          \
        switch (src) {                 \
            RPT_SRC(RPV, RP_ADMM64)    \
            RPT_SRC(RPV, RP_STORED64)  \
            default:                   \
                hipLaunchKernelGGL((k_report<RPV, RP_ZERO>), grid, block, 0, st, a); \
                break;                 \
        }                              \
        break;
    switch (g.RP) {
        RPT_CASE(16)
        RPT_CASE(32)
        RPT_CASE(48)
        RPT_CASE(64)
        RPT_CASE(128)
        RPT_CASE(256)
        default:
            throw Error(TRITD_ERR_UNSUPPORTED, "rank not supported by the report");
    }
#undef RPT_CASE
#undef RPT_SRC
    TRITD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_report_reduce, dim3((unsigned)cdiv(g.n3, 16) + 1), dim3(256), 0, st, a.part,
                       a.fpart, (int64_t)nb, g.n3, sums6, frame_sq);
    TRITD_CHECK_LAUNCH();
}

void run_report(const Geom& g, int src, RpArgs a, const ReportCall& c, hipStream_t st,
                double* kernel_ms) {
    const int64_t rows = g.n1l, cols = g.n2 * g.n3;
    const size_t ne = (size_t)(rows * cols);
    const bool ssim = c.frame_ssim != nullptr;
    const bool small = g.n1 < 11 || g.n2 < 11;  // ssim_index: -Inf below the window
    // k_ssim_tiles reads contiguous frames: a device X with spare rows is packed
    const bool packX = !c.on_device || (ssim && !small && c.ldX != rows);
    const bool packM = c.missing && !c.on_device;
    const int nb = report_grid(g);
    // ---- every allocation first ----
    DBuf dX, dM, part, fpart, out, dL, dw, sscr;
    if (packX) dX.alloc(ne);
    if (packM) dM.alloc_bytes(ne);
    part.alloc(6 * (size_t)nb);
    fpart.alloc((size_t)nb * (size_t)g.n3);
    out.alloc(6 + 2 * (size_t)g.n3);
    if (ssim) {
        if (!small) dL.alloc(ne);
        dw.alloc(121);
        sscr.alloc(ssim_scratch(g.n1, g.n2, g.n3));
    }
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) hip_quiet(hipEventDestroy(x));
        }
    } ev;
    if (kernel_ms)
        for (hipEvent_t& x : ev.e) TRITD_HIP(hipEventCreate(&x));
    // ---- staging ----
    a.X = c.X; a.ldX = c.ldX; a.missing = c.missing; a.ldM = c.ldM;
    auto pack = [&](void* dst, const void* src_, int64_t ld, size_t es) {
        const hipMemcpyKind kind = c.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (ld == rows)  // a whole tensor: one contiguous copy
            TRITD_HIP(hipMemcpyAsync(dst, src_, ne * es, kind, st));
        else
            TRITD_HIP(hipMemcpy2DAsync(dst, (size_t)rows * es, src_, (size_t)ld * es,
                                       (size_t)rows * es, (size_t)cols, kind, st));
    };
    if (packX) {
        pack(dX.p, c.X, c.ldX, sizeof(double));
        a.X = dX.p;
        a.ldX = rows;
    }
    if (packM) {
        pack(dM.p, c.missing, c.ldM, 1);
        a.missing = reinterpret_cast<const uint8_t*>(dM.p);
        a.ldM = rows;
    }
    if (ssim) TRITD_HIP(hipMemcpyAsync(dw.p, c.win, 121 * sizeof(double), hipMemcpyHostToDevice, st));
    a.part = part.p;
    a.fpart = fpart.p;
    a.Lout = dL.p;
    double* dsums = out.p;
    double* dfsq = out.p + 6;
    double* dss = out.p + 6 + g.n3;
    // ---- the pass ----
    if (kernel_ms) TRITD_HIP(hipEventRecord(ev.e[0], st));
    launch_report(g, src, a, dsums, dfsq, st);
    if (ssim) {
        const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
        // small: the finish alone writes -Inf; X and L are not read
        launch_ssim(a.X, dL.p, g.n1, g.n2, g.n3, dw.p, C1, C2, sscr.p, dss, st);
    }
    if (kernel_ms) TRITD_HIP(hipEventRecord(ev.e[1], st));
    // ---- results ----
    std::vector<double> h(6 + 2 * (size_t)g.n3);
    TRITD_HIP(hipMemcpyAsync(h.data(), out.p, (6 + (ssim ? 2 : 1) * (size_t)g.n3) * sizeof(double),
                             hipMemcpyDeviceToHost, st));
    TRITD_HIP(hipStreamSynchronize(st));
    if (c.sums) std::copy(h.begin(), h.begin() + 6, c.sums);
    if (c.frame_sq) std::copy(h.begin() + 6, h.begin() + 6 + g.n3, c.frame_sq);
    if (ssim) std::copy(h.begin() + 6 + g.n3, h.end(), c.frame_ssim);
    if (kernel_ms) {
        float ms = 0.0f;
        TRITD_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *kernel_ms = (double)ms;
    }
}

}  // namespace tritd
