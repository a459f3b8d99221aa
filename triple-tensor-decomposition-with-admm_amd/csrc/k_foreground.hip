// Foreground detection: eval of video_triple_comparison.m:316-371.
//
//   p = abs(F) > thr                                   :333,:339 (strict; NaN false)
//   g = (G == 255), m = (G == 170)                     :342-343
//   per frame  TP = #(p & (g|m))   FP = #(p & ~g)      :351-352
//              FN = #(~p & g)      TN = #(~p & (~g|m)) :353-354
//
// One streaming pass gives the mask bytes and the per-frame counts; the
// foreground F is never materialised when it lives in a session:
//   FG_ADMM64 / FG_ADMM32: F = O_k of an ADMM session, which K5 does not store,
//       formed per element from the resident D, Y_L (tile-major) and T (TX
//       order) by the expression k_o_fixup shares (o_expr.h);
//   FG_STORED64: a stored tile-major tensor (the nonconvex AlsSession's O);
//   FG_ZERO: no iteration has run, O = 0 and p is false everywhere (the
//       counts are then those of ~p);
//   k_fg_cm: a plain column-major F with a leading dimension (the primitives).
//
// Tile-major walk (k_fg_tm).  The ij-tile ordinal g = (j*n1p + i)/16 runs
// along the column-major plane of a frame, so a workgroup that takes FG_NT
// consecutive ij-tiles of one t-tile owns, for each of its 16 frames, one run
// of 16*FG_NT consecutive padded rows.  Phase 1: wave w takes tiles w, w+4, ...
// of the run; a lane loads its four elements the way K5 holds them (two 16 B
// loads per tensor in fp64, one in fp32; T by element in TX order) and writes
// the four predicate bytes to the LDS image P[t%16][row].  Phase 2: wave w owns
// frames 4w..4w+3 of the t-tile; a lane takes 16 consecutive rows of the run:
// one 16 B LDS read, one 16 B load of G, one 16 B store of pred, the four
// counts by byte-parallel compares and popcounts.  The counts are summed over
// the wave, and one lane adds them to counts[t][0..3]: one integer atomic per
// frame and count per workgroup, in any order the same sums.  Padding rows
// (i >= n1l), padded frames (t >= n3) and the tiles that pad a group of four
// are neither written nor counted.  The 16 B form needs n1l == n1p == ldG ==
// ldP and 16 B aligned pointers (a whole tensor whose n1 is a multiple of 16,
// every host-staged call with such a shard); otherwise phase 2 moves bytes,
// consecutive lanes on consecutive rows.
#include "kernels.h"
#include "o_expr.h"

namespace tritd {

typedef double d2v __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

constexpr int FG_NT = 64;                  // ij-tiles per workgroup: 1024 rows = 64 lanes x 16 B
constexpr int FG_ROW = 16 * FG_NT + 16;    // bytes of one frame's LDS row (+16: the four t a lane
                                           // writes fall in distinct banks)
static_assert(16 * FG_NT == 64 * 16, "phase 2 takes one 16-byte chunk per lane");

// 0x80 in every byte of v that is zero (exact: no carry crosses a byte)
__device__ __forceinline__ unsigned zero_bytes(unsigned v) {
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

// the four counts of four pixels: p holds 0/1 per byte, G the label bytes
__device__ __forceinline__ void fg_count4(unsigned p, unsigned G, unsigned (&c)[4]) {
    const unsigned g = zero_bytes(G ^ 0xFFFFFFFFu) >> 7;  // G == 255
    const unsigned m = zero_bytes(G ^ 0xAAAAAAAAu) >> 7;  // G == 170
    const unsigned np = p ^ 0x01010101u, ng = g ^ 0x01010101u;
    c[0] += __builtin_popcount(p & (g | m));
    c[1] += __builtin_popcount(p & ng);
    c[2] += __builtin_popcount(np & g);
    c[3] += __builtin_popcount(np & (ng | m));
}
__device__ __forceinline__ void fg_count1(unsigned p, unsigned G, unsigned (&c)[4]) {
    const unsigned g = G == 255u, m = G == 170u, np = p ^ 1u, ng = g ^ 1u;
    c[0] += p & (g | m);
    c[1] += p & ng;
    c[2] += np & g;
    c[3] += np & (ng | m);
}

// sum over the wave; lane 0 adds the four sums to counts[0..3]
__device__ __forceinline__ void fg_wave_add(unsigned (&c)[4], int lane, unsigned long long* counts) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned v = c[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off);
        if (lane == 0 && v) atomicAdd(counts + q, (unsigned long long)v);
    }
}

__device__ __forceinline__ unsigned char fg_pred(double v, double thr) {
    return __builtin_fabs(v) > thr ? 1 : 0;  // NaN: false; +-Inf: true
}

template <int SRC>
__global__ __launch_bounds__(256) void k_fg_tm(FgArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char P[16 * FG_ROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tt = (int64_t)blockIdx.x % a.ntt, run = (int64_t)blockIdx.x / a.ntt;
    const int64_t g0 = run * FG_NT;
    const int nt = (int)(a.tiles - g0 < FG_NT ? a.tiles - g0 : FG_NT);  // real tiles of the run
    const int il = lane & 15, tq = lane >> 4;

    // ---- phase 1: the predicate bytes of the run's tiles into P[t%16][row] ----
    if (SRC == FG_ZERO) {
        for (int q = threadIdx.x; q < 16 * FG_ROW / 16; q += 256)
            reinterpret_cast<u4*>(P)[q] = u4{0u, 0u, 0u, 0u};
    } else {
#pragma unroll 2
        for (int k = wave; k < nt; k += 4) {
            const int64_t base = tm_tile_base(g0 + k, tt, a.ntt);
            unsigned char* col = P + 16 * k + il;
            if (SRC == FG_ADMM32) {
                // lane l holds t%16 = 4(l>>4) + r, r = 0..3, of row l&15 at floats 4l..4l+3;
                // T: lane ((i&3)<<4)|t, slot i>>2 (k_o_fixup32)
                const f4 d = *reinterpret_cast<const f4*>(static_cast<const float*>(a.D) + base + 4 * lane);
                const f4 y = *reinterpret_cast<const f4*>(static_cast<const float*>(a.YL) + base + 4 * lane);
                const float* T = static_cast<const float*>(a.T) + base;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tl = 4 * tq + r;
                    const int tx = 4 * (((il & 3) << 4) | tl) + (il >> 2);
                    const float v = o_value32(d[r], y[r], T[tx], a.invL_next32);
                    col[tl * FG_ROW] = fg_pred((double)v, a.thr);
                }
            } else {
                // register r of lane l: t%16 = (l>>4) + 4r, row l&15, at (r>>1)*128 + 2l + (r&1);
                // T: slot s = i>>2 of lane ((i&3)<<4)|t at (s>>1)*128 + 2 lane + (s&1) (k_o_fixup)
                const double* D = static_cast<const double*>(a.D) + base;
                const d2v d0 = *reinterpret_cast<const d2v*>(D + 2 * lane);
                const d2v d1 = *reinterpret_cast<const d2v*>(D + 128 + 2 * lane);
                double v[4] = {d0[0], d0[1], d1[0], d1[1]};
                if (SRC == FG_ADMM64) {
                    const double* Y = static_cast<const double*>(a.YL) + base;
                    const d2v y0 = *reinterpret_cast<const d2v*>(Y + 2 * lane);
                    const d2v y1 = *reinterpret_cast<const d2v*>(Y + 128 + 2 * lane);
                    const double y[4] = {y0[0], y0[1], y1[0], y1[1]};
                    const double* T = static_cast<const double*>(a.T) + base;
                    const int s = il >> 2;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int tl = tq + 4 * r;
                        const int lx = ((il & 3) << 4) | tl;
                        const double t = T[((s >> 1) << 7) + (lx << 1) + (s & 1)];
                        const bool obs = !a.M || ((a.M[((base >> 8) << 2) + r] >> lane) & 1ull);
                        v[r] = o_value(v[r], y[r], t, a.invL_next, obs);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) col[(tq + 4 * r) * FG_ROW] = fg_pred(v[r], a.thr);
            }
        }
    }
    __syncthreads();

    // ---- phase 2: frames 4 wave .. 4 wave + 3 of the t-tile ----
    const int64_t row0 = g0 << 4;
    const int nrows = nt << 4;
    const int64_t plane = a.n1p * a.n2;
    for (int q = 0; q < 4; ++q) {
        const int tl = 4 * wave + q;
        const int64_t t = 16 * tt + tl;
        if (t >= a.n3) break;  // (wave-uniform)
        const unsigned char* prow = P + tl * FG_ROW;
        unsigned c[4] = {0u, 0u, 0u, 0u};
        if (a.vec) {  // n1l == n1p == ldG == ldP: the run is one contiguous, aligned piece
            if (16 * lane < nrows) {
                const int64_t off = t * plane + row0 + 16 * lane;
                const u4 p = *reinterpret_cast<const u4*>(prow + 16 * lane);
                if (a.pred) *reinterpret_cast<u4*>(a.pred + off) = p;
                if (a.gt) {
                    const u4 G = *reinterpret_cast<const u4*>(a.gt + off);
#pragma unroll
                    for (int w = 0; w < 4; ++w) fg_count4(p[w], G[w], c);
                }
            }
        } else {
            for (int r = lane; r < nrows; r += 64) {
                const int64_t row = row0 + r;
                const int64_t j = row / a.n1p, i = row - j * a.n1p;
                if (i >= a.n1l) continue;
                const unsigned p = prow[r];
                if (a.pred) a.pred[(t * a.n2 + j) * a.ldP + i] = (unsigned char)p;
                if (a.gt) fg_count1(p, a.gt[(t * a.n2 + j) * a.ldG + i], c);
            }
        }
        if (a.gt) fg_wave_add(c, lane, a.counts + 4 * t);
    }
}

void launch_foreground_tm(const Geom& g, int src, const FgArgs& in, hipStream_t st) {
    if (g.n1l <= 0) return;
    FgArgs a = in;
    a.n1l = g.n1l; a.n1p = g.n1p; a.n2 = g.n2; a.n3 = g.n3; a.tiles = g.tiles; a.ntt = g.ntt;
    auto ok = [&](const void* p, int64_t ld) {
        return !p || (ld == g.n1p && (reinterpret_cast<uintptr_t>(p) & 15u) == 0);
    };
    a.vec = g.n1l == g.n1p && ok(a.gt, a.ldG) && ok(a.pred, a.ldP);
    const int64_t grid = cdiv(g.tiles, FG_NT) * g.ntt;
    if (grid > 0x7fffffffll) throw Error(TRITD_ERR_UNSUPPORTED, "foreground: shard too large");
    const dim3 G((unsigned)grid), B(256);
    switch (src) {
        case FG_ADMM64: hipLaunchKernelGGL(k_fg_tm<FG_ADMM64>, G, B, 0, st, a); break;
        case FG_ADMM32: hipLaunchKernelGGL(k_fg_tm<FG_ADMM32>, G, B, 0, st, a); break;
        case FG_STORED64: hipLaunchKernelGGL(k_fg_tm<FG_STORED64>, G, B, 0, st, a); break;
        default: hipLaunchKernelGGL(k_fg_tm<FG_ZERO>, G, B, 0, st, a); break;
    }
    TRITD_CHECK_LAUNCH();
}

// Plain column-major F(i,j,t) = F[i + ldF (j + n2 t)], G and pred likewise.  A
// workgroup takes FG_CM elements of one frame's n1 x n2 plane: coalesced
// loads of F, the predicate bytes through LDS, then 16 elements per thread as
// above (16 B moves when the three leading dimensions equal n1, n1 n2 is a
// multiple of 16 and the byte pointers are aligned; bytes otherwise).
constexpr int FG_CM = 4096;

template <class T>
__global__ __launch_bounds__(256) void k_fg_cm(const T* __restrict__ F, int64_t ldF,
                                               const unsigned char* __restrict__ gt, int64_t ldG,
                                               unsigned char* __restrict__ pred, int64_t ldP,
                                               unsigned long long* counts, int64_t n1, int64_t n2,
                                               int64_t chunks, double thr, int vec) {
    __shared__ __attribute__((aligned(16))) unsigned char P[FG_CM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t t = (int64_t)blockIdx.x / chunks, ch = (int64_t)blockIdx.x % chunks;
    const int64_t ne = n1 * n2, e0 = ch * FG_CM;
    const bool flatF = ldF == n1;
#pragma unroll 4
    for (int k = 0; k < FG_CM / 256; ++k) {
        const int64_t e = e0 + k * 256 + tid;
        if (e >= ne) break;
        int64_t off = e;
        if (!flatF) {
            const int64_t j = e / n1;
            off = j * ldF + (e - j * n1);
        }
        P[k * 256 + tid] = fg_pred((double)F[t * n2 * ldF + off], thr);
    }
    __syncthreads();
    unsigned c[4] = {0u, 0u, 0u, 0u};
    const int64_t e = e0 + 16 * tid;
    if (vec) {  // ne % 16 == 0: a chunk of 16 is whole or absent
        if (e < ne) {
            const u4 p = *reinterpret_cast<const u4*>(P + 16 * tid);
            if (pred) *reinterpret_cast<u4*>(pred + t * ne + e) = p;
            if (gt) {
                const u4 G = *reinterpret_cast<const u4*>(gt + t * ne + e);
#pragma unroll
                for (int w = 0; w < 4; ++w) fg_count4(p[w], G[w], c);
            }
        }
    } else {
        // consecutive lanes on consecutive elements: element k*256 + tid of the chunk
        for (int k = 0; k < FG_CM / 256; ++k) {
            const int64_t x = e0 + k * 256 + tid;
            if (x >= ne) break;
            const int64_t j = x / n1, i = x - j * n1;
            const unsigned p = P[k * 256 + tid];
            if (pred) pred[(t * n2 + j) * ldP + i] = (unsigned char)p;
            if (gt) fg_count1(p, gt[(t * n2 + j) * ldG + i], c);
        }
    }
    if (gt) fg_wave_add(c, lane, counts + 4 * t);
}

void launch_foreground_cm(const void* F, bool f32, int64_t ldF, const uint8_t* gt, int64_t ldG,
                          uint8_t* pred, int64_t ldP, unsigned long long* counts, int64_t n1,
                          int64_t n2, int64_t nf, double thr, hipStream_t st) {
    const int64_t ne = n1 * n2, chunks = cdiv(ne, FG_CM);
    if (chunks * nf > 0x7fffffffll) throw Error(TRITD_ERR_UNSUPPORTED, "foreground: tensor too large");
    auto ok = [&](const void* p, int64_t ld) {
        return !p || (ld == n1 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0);
    };
    const int vec = (ne & 15) == 0 && ok(gt, ldG) && ok(pred, ldP);
    const dim3 G((unsigned)(chunks * nf)), B(256);
    if (f32)
        hipLaunchKernelGGL(k_fg_cm<float>, G, B, 0, st, static_cast<const float*>(F), ldF, gt, ldG,
                           pred, ldP, counts, n1, n2, chunks, thr, vec);
    else
        hipLaunchKernelGGL(k_fg_cm<double>, G, B, 0, st, static_cast<const double*>(F), ldF, gt, ldG,
                           pred, ldP, counts, n1, n2, chunks, thr, vec);
    TRITD_CHECK_LAUNCH();
}

// The host side of one call, shared by the sessions and the primitives: stage
// a host G in, zero the device counts, run `launch` (which receives the device
// G, pred and counts with their leading dimensions), bring pred and the counts
// back, and wait for the stream.  rows x cols: the byte planes (cols = n2 n3
// fibres of `rows` bytes).  kernel_ms (or null): the kernel's own time, from
// events around its launch.
void run_foreground(int64_t rows, int64_t cols, int64_t nf, const uint8_t* gt, int64_t ldG,
                    uint8_t* pred, int64_t ldP, int64_t* counts, bool on_device, hipStream_t st,
                    const std::function<void(const uint8_t*, int64_t, uint8_t*, int64_t,
                                             unsigned long long*)>& launch,
                    double* kernel_ms) {
    DBuf dg, dp, dc;
    struct Events {  // around the kernel alone, when its time is asked for
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) hip_quiet(hipEventDestroy(x));
        }
    } ev;
    if (kernel_ms)
        for (hipEvent_t& x : ev.e) TRITD_HIP(hipEventCreate(&x));
    const uint8_t* kgt = gt;
    uint8_t* kpred = pred;
    int64_t kldG = ldG, kldP = ldP;
    const size_t nb = (size_t)(rows * cols);
    if (gt && !on_device) {
        dg.alloc_bytes(nb);
        if (ldG == rows)  // a whole tensor: one contiguous copy
            TRITD_HIP(hipMemcpyAsync(dg.p, gt, nb, hipMemcpyHostToDevice, st));
        else
            TRITD_HIP(hipMemcpy2DAsync(dg.p, (size_t)rows, gt, (size_t)ldG, (size_t)rows,
                                       (size_t)cols, hipMemcpyHostToDevice, st));
        kgt = reinterpret_cast<const uint8_t*>(dg.p);
        kldG = rows;
    }
    if (pred && !on_device) {
        dp.alloc_bytes(nb);
        kpred = reinterpret_cast<uint8_t*>(dp.p);
        kldP = rows;
    }
    unsigned long long* kc = nullptr;
    if (gt) {
        dc.alloc(4 * (size_t)nf);
        kc = reinterpret_cast<unsigned long long*>(dc.p);
        TRITD_HIP(hipMemsetAsync(kc, 0, 4 * (size_t)nf * sizeof(unsigned long long), st));
    }
    if (kernel_ms) TRITD_HIP(hipEventRecord(ev.e[0], st));
    launch(kgt, kldG, kpred, kldP, kc);
    if (kernel_ms) TRITD_HIP(hipEventRecord(ev.e[1], st));
    if (pred && !on_device) {
        if (ldP == rows)
            TRITD_HIP(hipMemcpyAsync(pred, kpred, nb, hipMemcpyDeviceToHost, st));
        else
            TRITD_HIP(hipMemcpy2DAsync(pred, (size_t)ldP, kpred, (size_t)rows, (size_t)rows,
                                       (size_t)cols, hipMemcpyDeviceToHost, st));
    }
    if (gt)
        TRITD_HIP(hipMemcpyAsync(counts, kc, 4 * (size_t)nf * sizeof(int64_t), hipMemcpyDeviceToHost,
                                 st));
    TRITD_HIP(hipStreamSynchronize(st));
    if (kernel_ms) {
        float ms = 0.0f;
        TRITD_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *kernel_ms = (double)ms;
    }
}

}  // namespace tritd
