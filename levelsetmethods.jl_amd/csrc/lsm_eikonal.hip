// lsm_eikonal.hip — eikonal_(ϕ, speed, width, cutoff) on the device: |∇T| = s = 1/F on the dense grid, first-order Godunov upwind,
// by the block-based Fast Iterative Method (Jeong & Whitaker 2008); ϕ := copysign(min(T, c), ϕ).  s ≡ 1: the signed distance over
// the whole grid in O(N); a speed: travel times.  DESIGN.md §7.15; tests/_eikonal_ref.py restates every operation, in this file's
// operation order (built with -ffp-contract=off: the device rounds as numpy does).  The rules:
//   * a node is frozen (its T is given by the seed kernel) or free (T starts at +inf); inside and outside are one non-negative T;
//     neighbours off the grid do not exist, whatever the boundary condition;
//   * the update G of a free node: a_d = min of the two neighbours along axis d; the axes sorted by (a_d, d); a0 the smallest,
//     τ = s·h of its axis; for k = 2, 3 while a0 + τ > a_k: with w = 1/h², δ = a − a0 over the first k axes, A = Σw, B = Σwδ,
//     C = Σ(wδ)δ − s², disc = B² − AC, stop if disc < 0, τ = (B + sqrt(disc))/A; G = a0 + τ.  The quadratic is solved for T − a0,
//     not for T: the un-shifted form cancels like (a/h)²;
//   * a free node takes T := G only when G < T: T never rises, the iteration ends on a finite grid.
// Kernels: ek_seed (pointwise: reads ϕ and the speed, counts what is refused, writes T and the frozen mask), ek_mark (the tiles
// that hold a free node next to a frozen one), ek_compact (tile flags → compact list, flags cleared), ek_tile (one workgroup per
// listed tile: the tile and a one-node halo of T in LDS, up to EK_PASSES Jacobi passes of G, the tile's changed nodes written
// back), ek_final (ϕ := copysign(min(T, c), ϕ); the only kernel that writes ϕ).
//
// The activation invariant.  The tiles of one launch run concurrently and read each other's boundary layer from global memory
// while it may be being written.  That is harmless because (1) T only decreases, and every node is written by its own tile's
// workgroup alone (a tile appears once in a list); (2) T is an aligned 8-byte word: a load sees a whole old or a whole new value;
// (3) a stale read only postpones an update: a tile whose layer at face f changed during a launch flags the neighbour across f
// for the next launch, whatever that neighbour read meanwhile, and a tile that still changed in its last pass flags itself.  The
// next list is empty only when no tile changed anything: every free node then satisfies T <= G of its neighbours as they are.
// There is no grid-wide barrier and no cooperative launch; the host reads the list's length after every launch and the loop is
// bounded by max_iters.  With a cutoff c a change to a value >= c flags nobody: G > min a, so what depends on it is > c as well.
#include <algorithm>
#include <cmath>

#include "lsm_handle.h"
#include "wave.h"

namespace lsm {

// the measured choices; a variant library for tools/eikonal_bench.py --variants is built with -DLSM_EK_PASSES=… /
// -DLSM_EK_TX=… -DLSM_EK_TY=… -DLSM_EK_TZ=…
#ifndef LSM_EK_PASSES
#define LSM_EK_PASSES 8
#endif
#ifndef LSM_EK_TX
#define LSM_EK_TX 8
#define LSM_EK_TY 8
#define LSM_EK_TZ 8
#endif
constexpr int EK_PASSES = LSM_EK_PASSES;  // Jacobi passes per visit of a tile: one tile edge
constexpr long long EK_MAX_BLOCKS = 1LL << 24;
enum { EK_NONFINITE = 0, EK_BADSPEED = 1, EK_FROZEN = 2, EK_CLAMPED = 3, EK_NSTAT = 4 };

template <int N> struct EkTile;
template <> struct EkTile<2> { static constexpr int X = 32, Y = 8, Z = 1; };
template <> struct EkTile<3> { static constexpr int X = LSM_EK_TX, Y = LSM_EK_TY, Z = LSM_EK_TZ; };

struct EkArgs {
    int n[3], nt[3];            // nodes and tiles per axis
    long long s1, s2, origin;   // the padded layout of ϕ
    long long nnode, ntile;
    double h[3], w[3];          // w = 1/(h·h)
    double width, c;            // width 0: the crossing seed; c: the cutoff (+inf: none)
    const double* speed;        // dense, n-shaped, axis 0 fastest; NULL: 1
};

// G (the header comment).  a[d]: the smaller neighbour along axis d, +inf where there is none
template <int N>
__device__ __forceinline__ double ek_update(const double ain[N], double s, const EkArgs& g) {
    double a[N], hh[N], ww[N];
#pragma unroll
    for (int d = 0; d < N; ++d) { a[d] = ain[d]; hh[d] = g.h[d]; ww[d] = g.w[d]; }
    // a stable sort: ties keep the lower axis first
#define EK_CSWAP(i, j)                                                                                  \
    if (a[i] > a[j]) {                                                                                  \
        double t = a[i]; a[i] = a[j]; a[j] = t; t = hh[i]; hh[i] = hh[j]; hh[j] = t; t = ww[i]; ww[i] = ww[j]; ww[j] = t; \
    }
    EK_CSWAP(0, 1)
    if (N > 2) {
        EK_CSWAP(1, N - 1)
        EK_CSWAP(0, 1)
    }
#undef EK_CSWAP
    const double a0 = a[0];
    double tau = s * hh[0];
    if (a0 + tau > a[1]) {                  // false when a0 or a[1] is +inf
        const double d1 = a[1] - a0;
        double A = ww[0] + ww[1], B = ww[1] * d1;
        const double q1 = (ww[1] * d1) * d1;
        double disc = B * B - A * (q1 - s * s);
        if (!(disc < 0.0)) {
            tau = (B + sqrt(disc)) / A;
            if (N > 2 && a0 + tau > a[N - 1]) {
                const double d2 = a[N - 1] - a0;
                A = A + ww[N - 1];
                B = B + ww[N - 1] * d2;
                disc = B * B - A * ((q1 + (ww[N - 1] * d2) * d2) - s * s);
                if (!(disc < 0.0)) tau = (B + sqrt(disc)) / A;
            }
        }
    }
    return a0 + tau;
}

// node i of the dense arrays → its coordinates and its place in ϕ's padded layout
template <int N>
__device__ __forceinline__ long long ek_coords(const EkArgs& a, long long i, int I[3]) {
    I[0] = (int)(i % a.n[0]);
    const long long r = i / a.n[0];
    I[1] = N > 2 ? (int)(r % a.n[1]) : (int)r;
    I[2] = N > 2 ? (int)(r / a.n[1]) : 0;
    return a.origin + I[0] + I[1] * a.s1 + I[2] * a.s2;
}

// pointwise: the frozen nodes and their T (the two seedings of include/lsm.h), the counts of what the host refuses.  Reads ϕ only.
template <int N>
__global__ void __launch_bounds__(256) ek_seed_kernel(EkArgs a, const void* __restrict__ phi, int f32, double* __restrict__ T,
                                                      unsigned char* __restrict__ frozen, unsigned long long* st) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool fr = false;
    if (i < a.nnode) {
        int I[3];
        const long long at = ek_coords<N>(a, i, I);
        const double p = ld_val(phi, at, f32);
        if (!isfinite(p)) atomicAdd(&st[EK_NONFINITE], 1ULL);
        double s = 1.0;
        if (a.speed) {
            const double F = a.speed[i];
            if (!(F > 0.0) || !isfinite(F)) atomicAdd(&st[EK_BADSPEED], 1ULL);
            s = 1.0 / F;
        }
        const double ap = fabs(p);
        const bool pos = p > 0.0;
        const long long stride[3] = {1, a.s1, a.s2};
        bool adjacent = false;
        double acc = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            double sig = INFINITY;
#pragma unroll
            for (int step = -1; step <= 1; step += 2) {
                const int j = I[d] + step;
                if (j < 0 || j >= a.n[d]) continue;
                const double pj = ld_val(phi, at + step * stride[d], f32);
                if (p != 0.0 && (((pj > 0.0) != pos) || pj == 0.0)) {     // signs are compared, never multiplied
                    const double sg = a.h[d] * (ap / (ap + fabs(pj)));
                    if (sg < sig) sig = sg;
                    adjacent = true;
                }
            }
            if (sig < INFINITY) acc = acc + 1.0 / (sig * sig);
        }
        double t = INFINITY;
        if (a.width > 0.0) {
            fr = adjacent || ap <= a.width;
            if (fr) t = ap;
        } else {
            fr = adjacent || p == 0.0;
            if (p == 0.0) t = 0.0;
            else if (adjacent) t = s / sqrt(acc);
        }
        T[i] = t;
        frozen[i] = fr ? 1 : 0;
    }
    const unsigned long long m = __ballot(fr);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st[EK_FROZEN], (unsigned long long)__popcll(m));
}

template <int N>
__device__ __forceinline__ long long ek_tile_of(const EkArgs& a, const int I[3]) {
    return (I[0] / EkTile<N>::X) + (long long)a.nt[0] * ((I[1] / EkTile<N>::Y) + (N > 2 ? (long long)a.nt[1] * (I[2] / EkTile<N>::Z) : 0LL));
}

// the first list: the tiles that hold a free node with a frozen axis neighbour (in the tile or across a face)
template <int N>
__global__ void __launch_bounds__(256) ek_mark_kernel(EkArgs a, const unsigned char* __restrict__ frozen, unsigned char* next) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nnode || frozen[i]) return;
    int I[3];
    ek_coords<N>(a, i, I);
    const long long stride[3] = {1, a.n[0], (long long)a.n[0] * a.n[1]};
    bool touch = false;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        if (I[d] > 0) touch = touch || frozen[i - stride[d]];
        if (I[d] + 1 < a.n[d]) touch = touch || frozen[i + stride[d]];
    }
    if (touch) next[ek_tile_of<N>(a, I)] = 1;
}

// tile flags → the compact list (in no particular order); the flags are cleared for the next launch.  *count is zero on entry.
__global__ void __launch_bounds__(256) ek_compact_kernel(unsigned char* next, long long ntile, int* __restrict__ list, unsigned* count) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool on = i < ntile && next[i];
    if (on) next[i] = 0;
    const unsigned k = wave_append(on, count);
    if (on) list[k] = (int)i;
}

// one workgroup per listed tile, one thread per node of the tile.  Every global index is checked against the grid: a partial
// tile's nodes beyond it, and the halo beyond a face, are +inf in LDS and are never written.
template <int N>
__global__ void __launch_bounds__(EkTile<N>::X * EkTile<N>::Y * EkTile<N>::Z)
ek_tile_kernel(EkArgs a, double* T, const unsigned char* __restrict__ frozen, const int* __restrict__ list, unsigned nlist, unsigned char* next) {
    constexpr int TX = EkTile<N>::X, TY = EkTile<N>::Y, TZ = EkTile<N>::Z, NT = TX * TY * TZ;
    constexpr int LX = TX + 2, LY = TY + 2, LZ = N > 2 ? TZ + 2 : 1;
    __shared__ double sT[LX * LY * LZ];
    __shared__ int sface[6];
    if (blockIdx.x >= nlist) return;
    const int tile = list[blockIdx.x];
    const int b[3] = {tile % a.nt[0], (tile / a.nt[0]) % a.nt[1], N > 2 ? tile / (a.nt[0] * a.nt[1]) : 0};
    const int o[3] = {b[0] * TX, b[1] * TY, b[2] * TZ};
    const int tid = threadIdx.x;
    if (tid < 6) sface[tid] = 0;
    for (int e = tid; e < LX * LY * LZ; e += NT) {
        const int gx = o[0] + e % LX - 1, gy = o[1] + (e / LX) % LY - 1, gz = N > 2 ? o[2] + e / (LX * LY) - 1 : 0;
        const bool in = gx >= 0 && gx < a.n[0] && gy >= 0 && gy < a.n[1] && gz >= 0 && gz < a.n[2];
        sT[e] = in ? T[gx + (long long)a.n[0] * (gy + (long long)a.n[1] * gz)] : INFINITY;
    }
    const int t[3] = {tid % TX, (tid / TX) % TY, tid / (TX * TY)};
    const int I[3] = {o[0] + t[0], o[1] + t[1], o[2] + t[2]};
    const bool in = I[0] < a.n[0] && I[1] < a.n[1] && I[2] < a.n[2];
    const long long gi = I[0] + (long long)a.n[0] * (I[1] + (long long)a.n[1] * I[2]);
    const bool free_node = in && !frozen[gi];
    const double s = free_node && a.speed ? 1.0 / a.speed[gi] : 1.0;
    const int le = (t[0] + 1) + LX * ((t[1] + 1) + (N > 2 ? LY * (t[2] + 1) : 0));
    __syncthreads();
    const double start = sT[le];
    double mine = start;
    int stay = 0;
    for (int pass = 0; pass < EK_PASSES; ++pass) {
        double g = INFINITY;
        if (free_node) {
            double av[N];
            av[0] = fmin(sT[le - 1], sT[le + 1]);
            av[1] = fmin(sT[le - LX], sT[le + LX]);
            if (N > 2) av[N - 1] = fmin(sT[le - LX * LY], sT[le + LX * LY]);
            g = ek_update<N>(av, s, a);
        }
        const bool take = g < mine;
        const bool live = take && g < a.c;      // a change to a value >= c wakes nobody
        __syncthreads();                        // every thread has read this pass's neighbours
        if (take) {
            mine = g;
            sT[le] = g;
            if (live) {
                if (t[0] == 0) sface[0] = 1;
                if (t[0] == TX - 1) sface[1] = 1;
                if (t[1] == 0) sface[2] = 1;
                if (t[1] == TY - 1) sface[3] = 1;
                if (N > 2 && t[2] == 0) sface[4] = 1;
                if (N > 2 && t[2] == TZ - 1) sface[5] = 1;
            }
        }
        stay = __syncthreads_or(live ? 1 : 0);
        if (!stay) break;
    }
    if (mine < start) T[gi] = mine;             // only free nodes of the grid get here
    if (tid == 0 && stay) next[tile] = 1;
    if (tid < 2 * N && sface[tid]) {
        const int d = tid >> 1, nb = b[d] + ((tid & 1) ? 1 : -1);
        const int tstride[3] = {1, a.nt[0], a.nt[0] * a.nt[1]};
        if (nb >= 0 && nb < a.nt[d]) next[tile + ((tid & 1) ? tstride[d] : -tstride[d])] = 1;
    }
}

// ϕ := copysign(min(T, c), ϕ), rounded to the storage type; the ghosts are left as they are
template <int N>
__global__ void __launch_bounds__(256) ek_final_kernel(EkArgs a, const double* __restrict__ T, void* phi, int f32, unsigned long long* st) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool clamped = false;
    if (i < a.nnode) {
        int I[3];
        const long long at = ek_coords<N>(a, i, I);
        const double t = T[i];
        clamped = t > a.c;
        st_val(phi, at, f32, copysign(clamped ? a.c : t, ld_val(phi, at, f32)));
    }
    const unsigned long long m = __ballot(clamped);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st[EK_CLAMPED], (unsigned long long)__popcll(m));
}

// ---- host side
struct EikonalWorkspace {
    DevBuf<double> T;                // one per node
    DevBuf<unsigned char> frozen;    // one per node
    DevBuf<unsigned char> next;      // one per tile: active in the next launch
    DevBuf<int> list;                // the compact list of active tiles
    DevBuf<unsigned> count;          // its length
    DevBuf<unsigned long long> st;   // EK_NSTAT counters
};
void eikonal_workspace_free(EikonalWorkspace* w) { delete w; }

// returns 0, 1 (invalid: *err says why), 2 (a HIP call failed) or 3 (max_iters launches did not empty the list); ϕ is written
// only on 0
int eikonal_run(int ndim, const int n[3], long long s1, long long s2, long long origin, const double h[3], void* phi, int f32, const double* speed,
                double width, double cutoff, long long max_iters, hipStream_t stream, long long stats[4], const char** err, EikonalWorkspace** workspace) {
    if (ndim != 2 && ndim != 3) { *err = "eikonal: 2-D and 3-D fields only"; return 1; }
    EkArgs a;
    a.nnode = 1; a.ntile = 1;
    long long sum_n = 0;
    for (int d = 0; d < 3; ++d) {
        const int edge = ndim == 2 ? (d == 0 ? EkTile<2>::X : d == 1 ? EkTile<2>::Y : 1) : (d == 0 ? EkTile<3>::X : d == 1 ? EkTile<3>::Y : EkTile<3>::Z);
        a.n[d] = d < ndim ? n[d] : 1;
        a.h[d] = d < ndim ? h[d] : 1.0;
        a.w[d] = 1.0 / (a.h[d] * a.h[d]);
        if (d < ndim && n[d] < 2) { *err = "eikonal: at least two nodes per dimension"; return 1; }
        a.nt[d] = (a.n[d] + edge - 1) / edge;
        a.nnode *= a.n[d];
        a.ntile *= a.nt[d];
        if (d < ndim) sum_n += a.n[d];
    }
    a.s1 = s1; a.s2 = ndim > 2 ? s2 : 0; a.origin = origin;
    a.width = width; a.c = cutoff; a.speed = speed;
    if (a.nnode > EK_MAX_BLOCKS * 256) { *err = "eikonal: the grid is too large for one launch"; return 1; }
    if (max_iters <= 0) max_iters = 2 * sum_n;

    if (!*workspace) *workspace = new EikonalWorkspace();   // the handle's, created by its first call; the buffers only grow
    EikonalWorkspace& W = **workspace;
    MOD_HIP(W.T.grow((size_t)a.nnode * sizeof(double)), "hipMalloc(arrival times)");
    MOD_HIP(W.frozen.grow((size_t)a.nnode), "hipMalloc(frozen mask)");
    MOD_HIP(W.next.grow((size_t)a.ntile), "hipMalloc(tile flags)");
    MOD_HIP(W.list.grow((size_t)a.ntile * sizeof(int)), "hipMalloc(tile list)");
    MOD_HIP(W.count.grow(sizeof(unsigned)), "hipMalloc(list length)");
    MOD_HIP(W.st.grow(EK_NSTAT * sizeof(unsigned long long)), "hipMalloc(statistics)");
    MOD_HIP(hipMemsetAsync(W.st.p, 0, EK_NSTAT * sizeof(unsigned long long), stream), "eikonal: memset");
    MOD_HIP(hipMemsetAsync(W.next.p, 0, (size_t)a.ntile, stream), "eikonal: memset");
    const unsigned nblk = (unsigned)((a.nnode + 255) / 256), tblk = (unsigned)((a.ntile + 255) / 256);
    const unsigned tile_threads = ndim == 2 ? EkTile<2>::X * EkTile<2>::Y : EkTile<3>::X * EkTile<3>::Y * EkTile<3>::Z;

    LSM_LAUNCH_ND(ndim, ek_seed_kernel, nblk, 256, stream, a, (const void*)phi, f32, W.T.p, W.frozen.p, W.st.p);
    unsigned long long st[EK_NSTAT] = {};
    MOD_HIP(hipGetLastError(), "eikonal: launch failed");
    MOD_HIP(hipMemcpyAsync(st, W.st.p, sizeof(st), hipMemcpyDeviceToHost, stream), "eikonal: validation");
    MOD_HIP(hipStreamSynchronize(stream), "eikonal: validation");
    // what the data is refused for: stats = {-(reason), offending nodes, 0, 0} (include/lsm.h)
    const char* why[3] = {"eikonal: phi must be finite", "eikonal: the speed must be finite and positive at every node",
                          "eikonal: phi has no interface (no node is zero or next to a change of sign)"};
    const int reason = st[EK_NONFINITE] ? 1 : st[EK_BADSPEED] ? 2 : !st[EK_FROZEN] ? 3 : 0;
    if (reason) {
        stats[0] = -reason;
        stats[1] = reason == 1 ? (long long)st[EK_NONFINITE] : reason == 2 ? (long long)st[EK_BADSPEED] : 0;
        stats[2] = stats[3] = 0;
        *err = why[reason - 1];
        return 1;
    }

    LSM_LAUNCH_ND(ndim, ek_mark_kernel, nblk, 256, stream, a, (const unsigned char*)W.frozen.p, W.next.p);
    long long iters = 0, visits = 0;
    unsigned nlist = 0;
    for (;;) {
        MOD_HIP(hipMemsetAsync(W.count.p, 0, sizeof(unsigned), stream), "eikonal: memset");
        hipLaunchKernelGGL(ek_compact_kernel, dim3(tblk), dim3(256), 0, stream, W.next.p, a.ntile, W.list.p, W.count.p);
        MOD_HIP(hipMemcpyAsync(&nlist, W.count.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream), "eikonal: list length");
        MOD_HIP(hipStreamSynchronize(stream), "eikonal: device error");
        if (nlist == 0 || iters >= max_iters) break;
        if ((long long)nlist > a.ntile) { *err = "eikonal: the tile list is longer than the grid has tiles"; return 2; }
        LSM_LAUNCH_ND(ndim, ek_tile_kernel, nlist, tile_threads, stream, a, W.T.p, (const unsigned char*)W.frozen.p, (const int*)W.list.p, nlist, W.next.p);
        ++iters;
        visits += nlist;
    }
    stats[0] = (long long)st[EK_FROZEN];
    stats[1] = iters;
    stats[2] = visits;
    stats[3] = 0;
    if (nlist != 0) { *err = "eikonal: the active list did not empty within max_iters outer iterations"; return 3; }
    LSM_LAUNCH_ND(ndim, ek_final_kernel, nblk, 256, stream, a, (const double*)W.T.p, phi, f32, W.st.p);
    MOD_HIP(hipGetLastError(), "eikonal: launch failed");
    MOD_HIP(hipMemcpyAsync(st, W.st.p, sizeof(st), hipMemcpyDeviceToHost, stream), "eikonal: statistics");
    MOD_HIP(hipStreamSynchronize(stream), "eikonal: device error");
    stats[3] = (long long)st[EK_CLAMPED];
    return 0;
}

}  // namespace lsm
