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
    DevBuf<unsigned long long> st;   // EK_NSTAT counters (EX_NSTAT for the extension)
    DevBuf<double> F;                // extend_run: the fp64 working copies of the K fields, K per node
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

// ---- extend_from_interface_(F, ϕ): ∇F·∇|ϕ| = 0 off a frozen set, first-order upwind in the key g = |ϕ|, on eikonal's tile lists
// (the rule: the comment at lsm_extend in include/lsm.h; tests/_extend_ref.py restates every operation).
// A free node's value is (Σ c_d·F_Jd)/(Σ c_d), c_d = w_d·(g_I − a_d), over the axes whose smaller neighbour key a_d is strictly below
// g_I (g = ϕ resp. −ϕ where the frozen set is a whole side of ϕ): the system is triangular in g, every entry is computed once, from final values, so the bits do not depend on the schedule.
// Kernels: ex_init (pointwise: reads ϕ and the fields, counts what is refused, writes g into the workspace's T, the fixed bytes —
// frozen, filled at the cutoff, orphan — and the fp64 working copies W, a quiet NaN where a value is still to be computed),
// ek_mark and ek_compact as they are, ex_tile (one workgroup per listed tile and group of up to EX_GROUP fields: g and the fields
// with a one-node halo in LDS, up to EK_PASSES Jacobi passes; an entry (node, k) is computed when none of its participating
// neighbours' F_k is NaN), ex_check (the entries that are still NaN: none, or a wake-up was missed), ex_write (the only kernel
// that writes the fields).
// The activation invariant is eikonal's with "T only decreases" replaced by "an entry goes from NaN to its final value once":
// a workgroup alone writes its tile's entries of its fields, each as one aligned 8-byte store; a concurrent load sees NaN or the
// final value; NaN only postpones: the writer flags the neighbour across the face for the next launch, and a tile that still set
// something in its last pass flags itself.  Readiness is tested per field on the values themselves, so there is no flag array
// and no ordering between stores to rely on.
enum { EX_NONFINITE = 0, EX_BADF = 1, EX_FROZEN = 2, EX_ORPHAN = 3, EX_FILLED = 4, EX_UNSET = 5, EX_NSTAT = 6 };
enum { EX_RULE = 0, EX_MASK = 1, EX_INSIDE = 2, EX_OUTSIDE = 3 };
enum { EX_NODES = 0, EX_INTERFACE = 1 };
constexpr int EX_MAXK = 8, EX_GROUP = 4;

struct ExArgs {
    EkArgs g;                    // the grid; width and c as eikonal's; speed unused
    int rule, source, K, f32;
    double fill;
    void* F[EX_MAXK];            // the fields, in ϕ's padded layout and storage type
    const unsigned char* mask;   // EX_MASK: dense, n-shaped, axis 0 fastest
};

// (Σ c_d·f_d)/(Σ c_d) over the participating axes, ascending, clamped to the range of the f_d by comparisons (not fmin/fmax: the
// sign of a zero goes one way only): the maximum principle holds in floating point, a constant comes back as it is
struct ExSum {
    double num = 0.0, den = 0.0, lo = INFINITY, hi = -INFINITY;
    __device__ __forceinline__ void add(double c, double f) {
        num = num + c * f;
        den = den + c;
        if (f < lo) lo = f;
        if (f > hi) hi = f;
    }
    __device__ __forceinline__ double value() const {
        double r = num / den;
        if (!(r >= lo)) r = lo;
        if (!(r <= hi)) r = hi;
        return r;
    }
};

// the key g: |ϕ|; under EX_INSIDE ϕ and under EX_OUTSIDE −ϕ: the same at the free nodes, every frozen node below every free one
__device__ __forceinline__ double ex_key(double p, int rule) { return rule == EX_INSIDE ? p : rule == EX_OUTSIDE ? -p : fabs(p); }

template <int N>
__global__ void __launch_bounds__(256) ex_init_kernel(ExArgs x, const void* __restrict__ phi, double* __restrict__ g, unsigned char* __restrict__ fixed,
                                                      double* __restrict__ W, unsigned long long* st) {
    const EkArgs& a = x.g;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool fr = false, orphan = false, filled = false, badf = false;
    if (i < a.nnode) {
        int I[3];
        const long long at = ek_coords<N>(a, i, I);
        const double p = ld_val(phi, at, x.f32);
        if (!isfinite(p)) atomicAdd(&st[EX_NONFINITE], 1ULL);
        const double ap = fabs(p);
        const double key = ex_key(p, x.rule);
        const bool pos = p > 0.0;
        const long long stride[3] = {1, a.s1, a.s2};
        bool adjacent = false, part = false;
        double sig[N], th[N];
        long long joff[N];
#pragma unroll
        for (int d = 0; d < N; ++d) {
            sig[d] = INFINITY; th[d] = 0.0; joff[d] = 0;
            double amin = INFINITY;
#pragma unroll
            for (int step = -1; step <= 1; step += 2) {
                const int j = I[d] + step;
                if (j < 0 || j >= a.n[d]) continue;
                const double pj = ld_val(phi, at + step * stride[d], x.f32);
                const double apj = fabs(pj), kj = ex_key(pj, x.rule);
                if (kj < amin) amin = kj;
                if (p != 0.0 && (((pj > 0.0) != pos) || pj == 0.0)) {     // ek_seed_kernel's crossing test
                    const double theta = ap / (ap + apj);
                    const double sg = a.h[d] * theta;
                    if (sg < sig[d]) { sig[d] = sg; th[d] = theta; joff[d] = step * stride[d]; }   // a tie: the − side
                    adjacent = true;
                }
            }
            part = part || amin < key;
        }
        if (x.rule == EX_RULE) fr = adjacent || (a.width > 0.0 ? ap <= a.width : p == 0.0);
        else if (x.rule == EX_MASK) fr = x.mask[i] != 0;
        else if (x.rule == EX_INSIDE) fr = p <= 0.0;
        else fr = p >= 0.0;
        filled = !fr && ap >= a.c;
        orphan = !fr && !filled && !part;
        const bool reseed = fr && adjacent && x.source == EX_INTERFACE;
        for (int k = 0; k < x.K; ++k) {
            double v = __builtin_nan("");
            if (fr || orphan) {
                const double fi = ld_val(x.F[k], at, x.f32);
                if (!isfinite(fi)) badf = true;
                v = fi;
                if (reseed) {                       // the value at the crossings, from the input fields
                    ExSum s;
#pragma unroll
                    for (int d = 0; d < N; ++d)
                        if (sig[d] < INFINITY) {
                            const double fj = ld_val(x.F[k], at + joff[d], x.f32);
                            s.add(1.0 / (sig[d] * sig[d]), fi + th[d] * (fj - fi));
                        }
                    v = s.value();
                }
            } else if (filled) {
                v = x.fill;
            }
            W[(long long)k * a.nnode + i] = v;
        }
        g[i] = key;
        fixed[i] = (fr || orphan || filled) ? 1 : 0;
    }
    const bool flags[4] = {badf, fr, orphan, filled};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const unsigned long long m = __ballot(flags[f]);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st[EX_BADF + f], (unsigned long long)__popcll(m));
    }
}

// one workgroup per listed tile (blockIdx.x) and group of KG fields (blockIdx.y), one thread per node.  Every global index is
// checked against the grid: a partial tile's nodes beyond it and the halo beyond a face hold g = +inf in LDS, take part in
// nothing and are never written.
template <int N, int KG>
__global__ void __launch_bounds__(EkTile<N>::X * EkTile<N>::Y * EkTile<N>::Z)
ex_tile_kernel(EkArgs a, int K, const double* __restrict__ g, double* W, const unsigned char* __restrict__ fixed, const int* __restrict__ list,
               unsigned nlist, unsigned char* next) {
    constexpr int TX = EkTile<N>::X, TY = EkTile<N>::Y, TZ = EkTile<N>::Z, NT = TX * TY * TZ;
    constexpr int LX = TX + 2, LY = TY + 2, LZ = N > 2 ? TZ + 2 : 1, L = LX * LY * LZ;
    __shared__ double sG[L];
    __shared__ double sF[KG][L];
    __shared__ int sface[6];
    if (blockIdx.x >= nlist) return;
    const int k0 = (int)blockIdx.y * KG;
    const int kc = K - k0 < KG ? K - k0 : KG;
    const int tile = list[blockIdx.x];
    const int b[3] = {tile % a.nt[0], (tile / a.nt[0]) % a.nt[1], N > 2 ? tile / (a.nt[0] * a.nt[1]) : 0};
    const int o[3] = {b[0] * TX, b[1] * TY, b[2] * TZ};
    const int tid = threadIdx.x;
    if (tid < 6) sface[tid] = 0;
    for (int e = tid; e < L; e += NT) {
        const int gx = o[0] + e % LX - 1, gy = o[1] + (e / LX) % LY - 1, gz = N > 2 ? o[2] + e / (LX * LY) - 1 : 0;
        const bool in = gx >= 0 && gx < a.n[0] && gy >= 0 && gy < a.n[1] && gz >= 0 && gz < a.n[2];
        const long long at = gx + (long long)a.n[0] * (gy + (long long)a.n[1] * gz);
        sG[e] = in ? g[at] : INFINITY;
#pragma unroll
        for (int k = 0; k < KG; ++k) sF[k][e] = in && k < kc ? W[(long long)(k0 + k) * a.nnode + at] : 0.0;
    }
    const int t[3] = {tid % TX, (tid / TX) % TY, tid / (TX * TY)};
    const int I[3] = {o[0] + t[0], o[1] + t[1], o[2] + t[2]};
    const bool in = I[0] < a.n[0] && I[1] < a.n[1] && I[2] < a.n[2];
    const long long gi = I[0] + (long long)a.n[0] * (I[1] + (long long)a.n[1] * I[2]);
    const bool free_node = in && !fixed[gi];
    const int le = (t[0] + 1) + LX * ((t[1] + 1) + (N > 2 ? LY * (t[2] + 1) : 0));
    __syncthreads();
    // the participating neighbours and their weights, once: a_d the smaller key of the two (a tie: the − side), taken iff a_d < g_I
    constexpr int lstride[3] = {1, LX, LX * LY};
    int off[N];
    double c[N];
    bool part[N];
    const double gI = sG[le];
#pragma unroll
    for (int d = 0; d < N; ++d) {
        const double lo = sG[le - lstride[d]], hi = sG[le + lstride[d]];
        const bool tl = lo <= hi;
        const double ad = tl ? lo : hi;
        part[d] = free_node && ad < gI;
        c[d] = a.w[d] * (gI - ad);
        off[d] = tl ? le - lstride[d] : le + lstride[d];
    }
    double mine[KG];
    unsigned pending = 0, done = 0;          // per field: still NaN; set during this visit
#pragma unroll
    for (int k = 0; k < KG; ++k) {
        mine[k] = sF[k][le];
        if (free_node && k < kc && mine[k] != mine[k]) pending |= 1u << k;
    }
    int stay = 0;
    for (int pass = 0; pass < EK_PASSES; ++pass) {
        unsigned got = 0;
#pragma unroll
        for (int k = 0; k < KG; ++k) {
            if (!(pending >> k & 1u)) continue;
            ExSum s;
            bool ready = true;
#pragma unroll
            for (int d = 0; d < N; ++d)
                if (part[d]) {
                    const double f = sF[k][off[d]];
                    ready = ready && f == f;
                    s.add(c[d], f);
                }
            if (ready) { mine[k] = s.value(); got |= 1u << k; }
        }
        __syncthreads();                        // every thread has read this pass's neighbours
        if (got) {
#pragma unroll
            for (int k = 0; k < KG; ++k)
                if (got >> k & 1u) sF[k][le] = mine[k];
            pending &= ~got;
            done |= got;
            if (t[0] == 0) sface[0] = 1;
            if (t[0] == TX - 1) sface[1] = 1;
            if (t[1] == 0) sface[2] = 1;
            if (t[1] == TY - 1) sface[3] = 1;
            if (N > 2 && t[2] == 0) sface[4] = 1;
            if (N > 2 && t[2] == TZ - 1) sface[5] = 1;
        }
        stay = __syncthreads_or(got ? 1 : 0);
        if (!stay) break;
    }
#pragma unroll
    for (int k = 0; k < KG; ++k)
        if (done >> k & 1u) W[(long long)(k0 + k) * a.nnode + gi] = mine[k];     // only free nodes of the grid get here
    if (tid == 0 && stay) next[tile] = 1;
    if (tid < 2 * N && sface[tid]) {
        const int d = tid >> 1, nb = b[d] + ((tid & 1) ? 1 : -1);
        const int tstride[3] = {1, a.nt[0], a.nt[0] * a.nt[1]};
        if (nb >= 0 && nb < a.nt[d]) next[tile + ((tid & 1) ? tstride[d] : -tstride[d])] = 1;
    }
}

// the entries that still hold the sentinel after the list emptied
__global__ void __launch_bounds__(256) ex_check_kernel(long long nnode, int K, const double* __restrict__ W, unsigned long long* st) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int unset = 0;
    if (i < nnode)
        for (int k = 0; k < K; ++k) {
            const double v = W[(long long)k * nnode + i];
            unset += v != v ? 1 : 0;
        }
    const int total = wave_sum(unset);
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(&st[EX_UNSET], (unsigned long long)total);
}

// F_k := W_k rounded to the storage type; the ghosts are left as they are
template <int N>
__global__ void __launch_bounds__(256) ex_write_kernel(ExArgs x, const double* __restrict__ W) {
    const EkArgs& a = x.g;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nnode) return;
    int I[3];
    const long long at = ek_coords<N>(a, i, I);
    for (int k = 0; k < x.K; ++k) st_val(x.F[k], at, x.f32, W[(long long)k * a.nnode + i]);
}

template <int N>
static void ex_launch_tiles(const EkArgs& a, int K, EikonalWorkspace& W, unsigned nlist, hipStream_t stream) {
    constexpr unsigned NT = EkTile<N>::X * EkTile<N>::Y * EkTile<N>::Z;
    if (K == 1)
        hipLaunchKernelGGL((ex_tile_kernel<N, 1>), dim3(nlist, 1), dim3(NT), 0, stream, a, K, (const double*)W.T.p, W.F.p, (const unsigned char*)W.frozen.p,
                           (const int*)W.list.p, nlist, W.next.p);
    else
        hipLaunchKernelGGL((ex_tile_kernel<N, EX_GROUP>), dim3(nlist, (K + EX_GROUP - 1) / EX_GROUP), dim3(NT), 0, stream, a, K, (const double*)W.T.p, W.F.p,
                           (const unsigned char*)W.frozen.p, (const int*)W.list.p, nlist, W.next.p);
}

// returns 0, 1 (invalid: *err says why), 2 (a HIP call failed) or 3 (the list did not empty within max_iters, or an entry was
// left unset: an internal error); the fields are written only on 0.  stats[5]: include/lsm.h
int extend_run(int ndim, const int n[3], long long s1, long long s2, long long origin, const double h[3], const void* phi, int f32, void* const* F, int K,
               int rule, const unsigned char* mask, double width, int source, double cutoff, double fill, long long max_iters, hipStream_t stream,
               long long stats[5], const char** err, EikonalWorkspace** workspace) {
    if (ndim != 2 && ndim != 3) { *err = "extend: 2-D and 3-D fields only"; return 1; }
    if (K < 1 || K > EX_MAXK) { *err = "extend: 1 to 8 fields"; return 1; }
    ExArgs x;
    EkArgs& a = x.g;
    a.nnode = 1; a.ntile = 1;
    long long sum_n = 0;
    for (int d = 0; d < 3; ++d) {
        const int edge = ndim == 2 ? (d == 0 ? EkTile<2>::X : d == 1 ? EkTile<2>::Y : 1) : (d == 0 ? EkTile<3>::X : d == 1 ? EkTile<3>::Y : EkTile<3>::Z);
        a.n[d] = d < ndim ? n[d] : 1;
        a.h[d] = d < ndim ? h[d] : 1.0;
        a.w[d] = 1.0 / (a.h[d] * a.h[d]);
        if (d < ndim && n[d] < 2) { *err = "extend: at least two nodes per dimension"; return 1; }
        a.nt[d] = (a.n[d] + edge - 1) / edge;
        a.nnode *= a.n[d];
        a.ntile *= a.nt[d];
        if (d < ndim) sum_n += a.n[d];
    }
    a.s1 = s1; a.s2 = ndim > 2 ? s2 : 0; a.origin = origin;
    a.width = width; a.c = cutoff; a.speed = nullptr;
    x.rule = rule; x.source = source; x.K = K; x.f32 = f32; x.fill = fill; x.mask = mask;
    for (int k = 0; k < EX_MAXK; ++k) x.F[k] = k < K ? F[k] : nullptr;
    if (a.nnode > EK_MAX_BLOCKS * 256) { *err = "extend: the grid is too large for one launch"; return 1; }
    if (max_iters <= 0) max_iters = 2 * sum_n;

    if (!*workspace) *workspace = new EikonalWorkspace();
    EikonalWorkspace& W = **workspace;
    MOD_HIP(W.T.grow((size_t)a.nnode * sizeof(double)), "hipMalloc(keys)");
    MOD_HIP(W.frozen.grow((size_t)a.nnode), "hipMalloc(fixed mask)");
    MOD_HIP(W.next.grow((size_t)a.ntile), "hipMalloc(tile flags)");
    MOD_HIP(W.list.grow((size_t)a.ntile * sizeof(int)), "hipMalloc(tile list)");
    MOD_HIP(W.count.grow(sizeof(unsigned)), "hipMalloc(list length)");
    MOD_HIP(W.st.grow(EX_NSTAT * sizeof(unsigned long long)), "hipMalloc(statistics)");
    MOD_HIP(W.F.grow((size_t)K * (size_t)a.nnode * sizeof(double)), "hipMalloc(working copies)");
    MOD_HIP(hipMemsetAsync(W.st.p, 0, EX_NSTAT * sizeof(unsigned long long), stream), "extend: memset");
    MOD_HIP(hipMemsetAsync(W.next.p, 0, (size_t)a.ntile, stream), "extend: memset");
    const unsigned nblk = (unsigned)((a.nnode + 255) / 256), tblk = (unsigned)((a.ntile + 255) / 256);

    LSM_LAUNCH_ND(ndim, ex_init_kernel, nblk, 256, stream, x, phi, W.T.p, W.frozen.p, W.F.p, W.st.p);
    unsigned long long st[EX_NSTAT] = {};
    MOD_HIP(hipGetLastError(), "extend: launch failed");
    MOD_HIP(hipMemcpyAsync(st, W.st.p, sizeof(st), hipMemcpyDeviceToHost, stream), "extend: validation");
    MOD_HIP(hipStreamSynchronize(stream), "extend: validation");
    // what the data is refused for: stats = {-(reason), offending nodes, 0, 0, 0} (include/lsm.h)
    const char* why[3] = {"extend: phi must be finite", "extend: every field must be finite at the frozen nodes", "extend: no node is frozen"};
    const int reason = st[EX_NONFINITE] ? 1 : st[EX_BADF] ? 2 : !st[EX_FROZEN] ? 3 : 0;
    for (int i = 0; i < 5; ++i) stats[i] = 0;
    if (reason) {
        stats[0] = -reason;
        stats[1] = reason == 1 ? (long long)st[EX_NONFINITE] : reason == 2 ? (long long)st[EX_BADF] : 0;
        *err = why[reason - 1];
        return 1;
    }

    LSM_LAUNCH_ND(ndim, ek_mark_kernel, nblk, 256, stream, a, (const unsigned char*)W.frozen.p, W.next.p);
    long long iters = 0, visits = 0;
    unsigned nlist = 0;
    for (;;) {
        MOD_HIP(hipMemsetAsync(W.count.p, 0, sizeof(unsigned), stream), "extend: memset");
        hipLaunchKernelGGL(ek_compact_kernel, dim3(tblk), dim3(256), 0, stream, W.next.p, a.ntile, W.list.p, W.count.p);
        MOD_HIP(hipMemcpyAsync(&nlist, W.count.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream), "extend: list length");
        MOD_HIP(hipStreamSynchronize(stream), "extend: device error");
        if (nlist == 0 || iters >= max_iters) break;
        if ((long long)nlist > a.ntile) { *err = "extend: the tile list is longer than the grid has tiles"; return 2; }
        if (ndim == 2) ex_launch_tiles<2>(a, K, W, nlist, stream);
        else ex_launch_tiles<3>(a, K, W, nlist, stream);
        ++iters;
        visits += nlist;
    }
    stats[0] = (long long)st[EX_FROZEN];
    stats[1] = iters;
    stats[2] = visits;
    stats[3] = (long long)st[EX_ORPHAN];
    stats[4] = (long long)st[EX_FILLED];
    if (nlist != 0) { *err = "extend: the active list did not empty within max_iters outer iterations"; return 3; }
    hipLaunchKernelGGL(ex_check_kernel, dim3(nblk), dim3(256), 0, stream, a.nnode, K, (const double*)W.F.p, W.st.p);
    MOD_HIP(hipGetLastError(), "extend: launch failed");
    MOD_HIP(hipMemcpyAsync(st, W.st.p, sizeof(st), hipMemcpyDeviceToHost, stream), "extend: statistics");
    MOD_HIP(hipStreamSynchronize(stream), "extend: device error");
    if (st[EX_UNSET]) { *err = "extend: internal error: the list emptied with entries left unset (a missed wake-up); the fields are untouched"; return 3; }
    LSM_LAUNCH_ND(ndim, ex_write_kernel, nblk, 256, stream, x, (const double*)W.F.p);
    MOD_HIP(hipGetLastError(), "extend: launch failed");
    MOD_HIP(hipStreamSynchronize(stream), "extend: device error");
    return 0;
}

}  // namespace lsm
