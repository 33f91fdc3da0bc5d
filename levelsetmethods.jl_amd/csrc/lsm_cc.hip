// lsm_cc.hip — components(ϕ, level, side) on the device: the connected components of {ϕ < level} (side 0) or of its complement
// (side 1) on the dense grid, their node counts, index sums and bounding boxes, and the flip that removes some of them.
// DESIGN.md §7.16; tests/_cc_ref.py restates the definition and the flip rule.  The rules:
//   * inside(I) := ϕ[I] < level (ϕ == level and NaN are outside), as in kuhn.h; f32 storage widens exactly;
//   * two set nodes are adjacent iff they differ by ±d, d ∈ {0,1}^N \ {0}: the edges of the Freudenthal (Kuhn) subdivision that
//     isosurface and volume_mesh cut (6 neighbours in 2-D, 14 in 3-D).  Every edge is visited once, from its lower end: the
//     forward offsets +d (3 in 2-D, 7 in 3-D);
//   * components are numbered 0 … K−1 by their smallest linear node index (axis 0 fastest).
// Block-based union–find.  parent[] holds one uint32 per node (CC_NONE off the set), with parent[x] <= x at all times:
//   cc_local   one workgroup per tile (8×8×8; 32×8 in 2-D): set flags and a union–find over the tile's inner edges in LDS;
//              parent[I] := the global index of the local root.  Counts the set nodes and the non-finite values.
//   cc_merge   the forward edges that leave a tile (faces, edges and the corner): a lock-free union on global memory.
//   cc_flatten parent[I] := root(I); counts the roots of every chunk of CC_CHUNK nodes.
//   chunk_scan exclusive scan of the chunk counts in one workgroup (scan.h); K.  The host reads K and the counters here: its one read.
//   cc_number  labels[r] := the rank of root r among the roots;  cc_init clears the K-sized statistics.
//   cc_label   one workgroup per tile: labels[I] := labels[parent[I]] or −1; the statistics are summed per label in an LDS hash
//              table first (a wave that holds one label adds once), then one global atomic per statistic and per (tile, label).
//   cc_flip_count / cc_flip_write   lsm_cc_flip's two passes.
//
// The union (cc_union) and why stale loads cannot break it.  To join a and b: walk both to a node that looks like a root
// (ra, rb); if they differ, hi = max, lo = min, old = atomicMin(&parent[hi], lo); old == hi: hi was a root at that instant and
// now hangs under lo: done; otherwise go on with the pair (old, lo).  Invariants: (1) parent[x] <= x, every store being an
// atomicMin with lo < hi: a walk strictly descends and ends; (2) every value parent[x] ever held is a node that the edges seen so
// far connect to x: a link x → q is only ever replaced by x → lo with lo < q, by a thread that then still owes the pair (q, lo).
// So the relation "linked now, or owed by a running thread" only grows, and contains every edge once all threads are done.  A
// walk over stale values (another CU's L1 may hold an old line: MI355X_MICROARCH.md, "Stale without an agent-scope acquire")
// follows links that once existed, so by (2) it still ends at a node of the same component; whether that node is a root NOW is
// decided by the value the atomicMin returns, never by a load.  A stale walk can cost a further round (the pair's maximum
// strictly falls every round, so the rounds are bounded), never a wrong or a missing union.  No thread waits for another: no
// flag, no barrier across workgroups, no cooperative launch.  When the kernel has ended every tree's root is its smallest
// index, whatever the schedule: labels and numbering are deterministic.  The walks use relaxed agent-scope atomic loads (they
// bypass the L1), which only makes stale values rare.
#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>

#include "kuhn.h"
#include "scan.h"

namespace lsm {

constexpr unsigned CC_NONE = 0xffffffffu;
constexpr int CC_CHUNK = KUHN_CHUNK;          // nodes per workgroup of the flatten and number kernels
constexpr int CC_PER = CC_CHUNK / 256;
enum { CC_SET = 0, CC_CROSS = 1, CC_NONFINITE = 2, CC_K = 3, CC_NSTAT = 4 };
enum { CC_FLAGGED = 0, CC_MISMATCH = 1 };

template <int N> struct CcTile;
template <> struct CcTile<2> { static constexpr int X = 32, Y = 8, Z = 1; };
template <> struct CcTile<3> { static constexpr int X = 8, Y = 8, Z = 8; };

struct CcArgs {
    int n[3], nt[3];            // nodes and tiles per axis
    long long s1, s2, origin;   // the padded layout of ϕ
    long long nnode, ntile, nchunk;
    double level;
    int side, f32;              // side 0: {ϕ < level}, 1: its complement
};

__device__ __forceinline__ bool cc_in_set(double v, double level, int side) { return (v < level) != (side != 0); }

template <bool LDS>
__device__ __forceinline__ unsigned cc_load(const unsigned* p) {
    return LDS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ unsigned cc_find(const unsigned* parent, unsigned x) {
    for (;;) {
        const unsigned q = cc_load<LDS>(parent + x);
        if (q >= x) return x;       // q == x: a root (q > x never happens: invariant 1)
        x = q;
    }
}
// the header comment
template <bool LDS>
__device__ __forceinline__ void cc_union(unsigned* parent, unsigned a, unsigned b) {
    for (;;) {
        a = cc_find<LDS>(parent, a);
        b = cc_find<LDS>(parent, b);
        if (a == b) return;
        const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
        const unsigned old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

// the workgroup's sum of x added to *dst by one atomic.  Every thread calls this.
__device__ __forceinline__ void cc_block_add(unsigned x, unsigned* s_tot, unsigned long long* dst) {
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(s_tot, x);
    __syncthreads();
    if (threadIdx.x == 0 && *s_tot) atomicAdd(dst, (unsigned long long)*s_tot);
}

template <int N>
struct CcPlace {     // a thread's node in a tile kernel
    int t[3], I[3];
    bool in;
    long long gi;
};
template <int N>
__device__ __forceinline__ CcPlace<N> cc_place(const CcArgs& a) {
    constexpr int TX = CcTile<N>::X, TY = CcTile<N>::Y;
    CcPlace<N> p;
    const long long tile = blockIdx.x;
    const int b[3] = {(int)(tile % a.nt[0]), (int)((tile / a.nt[0]) % a.nt[1]), N > 2 ? (int)(tile / ((long long)a.nt[0] * a.nt[1])) : 0};
    const int tid = threadIdx.x;
    p.t[0] = tid % TX; p.t[1] = (tid / TX) % TY; p.t[2] = tid / (TX * TY);
    p.I[0] = b[0] * TX + p.t[0]; p.I[1] = b[1] * TY + p.t[1]; p.I[2] = b[2] * CcTile<N>::Z + p.t[2];
    p.in = p.I[0] < a.n[0] && p.I[1] < a.n[1] && p.I[2] < a.n[2];
    p.gi = p.I[0] + (long long)a.n[0] * (p.I[1] + (long long)a.n[1] * p.I[2]);
    return p;
}

// one workgroup per tile, one thread per node of the tile; a partial tile's nodes beyond the grid are off the set and are
// never addressed in global memory
template <int N>
__global__ void __launch_bounds__(CcTile<N>::X * CcTile<N>::Y * CcTile<N>::Z)
cc_local_kernel(CcArgs a, const void* __restrict__ phi, unsigned* __restrict__ parent, unsigned long long* st) {
    constexpr int TX = CcTile<N>::X, TY = CcTile<N>::Y, TZ = CcTile<N>::Z, NT = TX * TY * TZ;
    __shared__ unsigned sp[NT];
    __shared__ unsigned s_tot[2];
    const CcPlace<N> p = cc_place<N>(a);
    const int tid = threadIdx.x;
    if (tid < 2) s_tot[tid] = 0;
    bool set = false, bad = false;
    if (p.in) {
        const double v = ld_val(phi, a.origin + p.I[0] + p.I[1] * a.s1 + p.I[2] * a.s2, a.f32);
        bad = !isfinite(v);
        set = cc_in_set(v, a.level, a.side);
    }
    sp[tid] = set ? (unsigned)tid : CC_NONE;
    __syncthreads();
    if (set) {
#pragma unroll
        for (int d = 1; d < (1 << N); ++d) {
            const int dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
            if (p.t[0] + dx >= TX || p.t[1] + dy >= TY || p.t[2] + dz >= TZ) continue;     // leaves the tile: cc_merge
            const int nb = tid + dx + TX * (dy + TY * dz);
            if (sp[nb] != CC_NONE) cc_union<true>(sp, (unsigned)tid, (unsigned)nb);        // off the grid is CC_NONE too
        }
    }
    __syncthreads();
    if (p.in) {
        unsigned out = CC_NONE;
        if (set) {
            // the tile's order and the grid's agree inside a tile: the local root is the piece's smallest linear index
            const int r = (int)cc_find<true>(sp, (unsigned)tid);
            const int rx = r % TX, ry = (r / TX) % TY, rz = r / (TX * TY);
            out = (unsigned)(p.gi + (rx - p.t[0]) + (long long)a.n[0] * ((ry - p.t[1]) + (long long)a.n[1] * (rz - p.t[2])));
        }
        parent[p.gi] = out;
    }
    cc_block_add(set ? 1u : 0u, &s_tot[0], &st[CC_SET]);
    cc_block_add(bad ? 1u : 0u, &s_tot[1], &st[CC_NONFINITE]);
}

// the forward edges that leave the tile, both ends in the set.  parent[] is complete: cc_local has ended.
template <int N>
__global__ void __launch_bounds__(CcTile<N>::X * CcTile<N>::Y * CcTile<N>::Z) cc_merge_kernel(CcArgs a, unsigned* parent, unsigned long long* st) {
    constexpr int TX = CcTile<N>::X, TY = CcTile<N>::Y, TZ = CcTile<N>::Z;
    __shared__ unsigned s_tot;
    const CcPlace<N> p = cc_place<N>(a);
    if (threadIdx.x == 0) s_tot = 0;
    __syncthreads();
    unsigned cross = 0;
    const bool edge = p.t[0] == TX - 1 || p.t[1] == TY - 1 || (N > 2 && p.t[2] == TZ - 1);
    // membership never changes after cc_local: a plain load decides it
    if (p.in && edge && parent[p.gi] != CC_NONE) {
#pragma unroll
        for (int d = 1; d < (1 << N); ++d) {
            const int dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
            if (p.t[0] + dx < TX && p.t[1] + dy < TY && p.t[2] + dz < TZ) continue;        // stays in the tile: cc_local did it
            if (p.I[0] + dx >= a.n[0] || p.I[1] + dy >= a.n[1] || p.I[2] + dz >= a.n[2]) continue;
            const long long gj = p.gi + dx + (long long)a.n[0] * (dy + (long long)a.n[1] * dz);
            if (parent[gj] == CC_NONE) continue;
            ++cross;
            cc_union<false>(parent, (unsigned)p.gi, (unsigned)gj);
        }
    }
    cc_block_add(cross, &s_tot, &st[CC_CROSS]);
}

// parent[i] := root(i), in place.  Another thread may store parent[r] while this one walks over it: the old value and the new
// are both ancestors of r, roots do not change in this kernel, and an aligned 4-byte word is never torn.
__global__ void __launch_bounds__(256) cc_flatten_kernel(CcArgs a, unsigned* parent, unsigned* __restrict__ sums) {
    __shared__ unsigned wsum[4];
    const long long c0 = (long long)blockIdx.x * CC_CHUNK;
    unsigned roots = 0;
#pragma unroll 4
    for (int k = 0; k < CC_PER; ++k) {
        const long long i = c0 + 256 * k + threadIdx.x;
        if (i >= a.nnode) break;
        unsigned r = parent[i];
        if (r == CC_NONE) continue;
        r = cc_find<false>(parent, r);
        parent[i] = r;
        roots += r == (unsigned)i;
    }
    roots = block_sum<4>(roots, wsum);
    if (threadIdx.x == 0) sums[blockIdx.x] = roots;
}

// labels[r] := the number of roots below r, for every root r, in the chunks of cc_flatten
__global__ void __launch_bounds__(256) cc_number_kernel(CcArgs a, const unsigned* __restrict__ parent, const unsigned* __restrict__ off, int* __restrict__ labels) {
    __shared__ unsigned wsum[4];
    const long long c0 = (long long)blockIdx.x * CC_CHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned base = off[blockIdx.x];
    for (int k = 0; k < CC_PER; ++k) {        // uniform over the workgroup: the barriers are reached by every thread
        const long long i = c0 + 256 * k + threadIdx.x;
        const bool root = i < a.nnode && parent[i] == (unsigned)i;
        const unsigned long long m = __ballot(root);
        if (lane == 0) wsum[wave] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        if (root) labels[i] = (int)(base + before + (unsigned)__popcll(m & ((1ULL << lane) - 1ULL)));
        base += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) cc_init_kernel(long long K, int ndim, long long* __restrict__ nodes, long long* __restrict__ sums, int* __restrict__ bbox) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    nodes[k] = 0;
    for (int d = 0; d < ndim; ++d) {
        sums[k * ndim + d] = 0;
        bbox[(k * 2 + 0) * ndim + d] = INT_MAX;
        bbox[(k * 2 + 1) * ndim + d] = INT_MIN;
    }
}

// One workgroup per tile.  A root's label is already in labels[] (cc_number) and is stored again unchanged, so the loads of
// other workgroups see the same value before and after.  Statistics: an LDS table of 2·NT slots keyed by the label (more slots
// than the tile has nodes: an insertion always finds one), holding the count, the sums of the in-tile coordinates and, per
// axis, a bit mask of the in-tile coordinates that occur (the bounding box).
template <int N>
__global__ void __launch_bounds__(CcTile<N>::X * CcTile<N>::Y * CcTile<N>::Z)
cc_label_kernel(CcArgs a, const unsigned* __restrict__ parent, int* labels, long long* nodes, long long* sums, int* bbox) {
    constexpr int TX = CcTile<N>::X, TY = CcTile<N>::Y, TZ = CcTile<N>::Z, NT = TX * TY * TZ, H = 2 * NT;
    __shared__ int s_key[H];
    __shared__ unsigned s_cnt[H], s_sum[N][H], s_occ[N][H];
    const CcPlace<N> p = cc_place<N>(a);
    const int tid = threadIdx.x;
    for (int e = tid; e < H; e += NT) {
        s_key[e] = -1;
        s_cnt[e] = 0;
#pragma unroll
        for (int d = 0; d < N; ++d) { s_sum[d][e] = 0; s_occ[d][e] = 0; }
    }
    int lab = -1;
    if (p.in) {
        const unsigned r = parent[p.gi];
        if (r != CC_NONE) lab = labels[r];
        labels[p.gi] = lab;
    }
    __syncthreads();
    // a wave that holds one label (the inside of a body) adds once
    const int first = __shfl(lab, 0, 64);
    const bool uniform = __all(lab == first);
    unsigned cnt = lab >= 0 ? 1u : 0u, sum[N], occ[N];
#pragma unroll
    for (int d = 0; d < N; ++d) { sum[d] = (unsigned)p.t[d]; occ[d] = 1u << p.t[d]; }
    if (uniform) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            cnt += __shfl_xor(cnt, s, 64);
#pragma unroll
            for (int d = 0; d < N; ++d) { sum[d] += __shfl_xor(sum[d], s, 64); occ[d] |= __shfl_xor(occ[d], s, 64); }
        }
    }
    if (lab >= 0 && (!uniform || (tid & 63) == 0)) {
        int slot = (int)(((unsigned)lab * 2654435761u) >> 16) & (H - 1);
        for (;;) {
            const int k = atomicCAS(&s_key[slot], -1, lab);
            if (k == -1 || k == lab) break;
            slot = (slot + 1) & (H - 1);
        }
        atomicAdd(&s_cnt[slot], cnt);
#pragma unroll
        for (int d = 0; d < N; ++d) { atomicAdd(&s_sum[d][slot], sum[d]); atomicOr(&s_occ[d][slot], occ[d]); }
    }
    __syncthreads();
    const int o[3] = {p.I[0] - p.t[0], p.I[1] - p.t[1], p.I[2] - p.t[2]};     // the tile's first node
    for (int e = tid; e < H; e += NT) {
        const int k = s_key[e];
        if (k < 0) continue;
        const long long c = s_cnt[e];
        atomicAdd((unsigned long long*)&nodes[k], (unsigned long long)c);
#pragma unroll
        for (int d = 0; d < N; ++d) {
            atomicAdd((unsigned long long*)&sums[(long long)k * N + d], (unsigned long long)(c * o[d] + (long long)s_sum[d][e]));
            const unsigned m = s_occ[d][e];
            atomicMin(&bbox[((long long)k * 2 + 0) * N + d], o[d] + (__ffs(m) - 1));
            atomicMax(&bbox[((long long)k * 2 + 1) * N + d], o[d] + (31 - __clz(m)));
        }
    }
}

// the neighbours of a finite value, by its bits (x == 0: the smallest subnormal of the wanted sign)
__device__ __forceinline__ double cc_next(double x, bool up) {
    if (x == 0.0) return up ? __longlong_as_double(1LL) : __longlong_as_double((long long)0x8000000000000001ULL);
    const long long b = __double_as_longlong(x);
    return __longlong_as_double((x > 0.0) == up ? b + 1 : b - 1);
}
__device__ __forceinline__ float cc_nextf(float x, bool up) {
    if (x == 0.0f) return up ? __int_as_float(1) : __int_as_float((int)0x80000001u);
    const int b = __float_as_int(x);
    return __int_as_float((x > 0.0f) == up ? b + 1 : b - 1);
}

template <int N>
__device__ __forceinline__ long long cc_padded(const CcArgs& a, long long i) {
    const int x = (int)(i % a.n[0]);
    const long long r = i / a.n[0];
    const int y = N > 2 ? (int)(r % a.n[1]) : (int)r, z = N > 2 ? (int)(r / a.n[1]) : 0;
    return a.origin + x + y * a.s1 + z * a.s2;
}

// the nodes of the flagged components, and those of them that ϕ no longer puts on the object's side.  Reads only.
template <int N>
__global__ void __launch_bounds__(256) cc_flip_count_kernel(CcArgs a, const void* __restrict__ phi, const int* __restrict__ labels,
                                                            const unsigned char* __restrict__ which, unsigned long long* cnt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool flagged = false, mismatch = false;
    if (i < a.nnode) {
        const int l = labels[i];
        if (l >= 0 && which[l]) {
            flagged = true;
            mismatch = !cc_in_set(ld_val(phi, cc_padded<N>(a, i), a.f32), a.level, a.side);
        }
    }
    const unsigned long long mf = __ballot(flagged), mm = __ballot(mismatch);
    if ((threadIdx.x & 63) == 0) {
        if (mf) atomicAdd(&cnt[CC_FLAGGED], (unsigned long long)__popcll(mf));
        if (mm) atomicAdd(&cnt[CC_MISMATCH], (unsigned long long)__popcll(mm));
    }
}

// v' = level + (level − v): two fp64 operations, no contraction (this file is built with -ffp-contract=off).  A node of
// {ϕ < level} lands on v' >= level as it is (level − v > 0); a node of the complement that does not land below level takes
// the double just below it.  f32 storage: rounded once, and moved to the neighbouring float on the right side where the
// rounding crossed the level.
template <int N>
__global__ void __launch_bounds__(256) cc_flip_write_kernel(CcArgs a, void* phi, const int* __restrict__ labels, const unsigned char* __restrict__ which) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nnode) return;
    const int l = labels[i];
    if (l < 0 || !which[l]) return;
    const long long at = cc_padded<N>(a, i);
    const double v = ld_val(phi, at, a.f32);
    const double diff = a.level - v;
    double w = a.level + diff;
    const bool below = a.side != 0;                 // the side the node has to land on: below level, or not below
    if (below && !(w < a.level)) w = cc_next(a.level, false);
    if (a.f32) {
        float f = (float)w;
        if (((double)f < a.level) != below) f = cc_nextf(f, !below);
        static_cast<float*>(phi)[at] = f;
    } else {
        static_cast<double*>(phi)[at] = w;
    }
}

// ---- host side
struct CcWorkspace {
    DevBuf<unsigned> parent;            // one per node
    DevBuf<unsigned> sums, off;         // one per chunk: roots, and their exclusive scan
    DevBuf<unsigned long long> st;      // CC_NSTAT counters, then lsm_cc_flip's two
};
void cc_workspace_free(CcWorkspace* w) { delete w; }

struct CcObject {
    CcArgs a;
    int ndim = 0;
    long long K = 0;
    DevBuf<int> labels;                 // one per node
    DevBuf<long long> nodes, sums;      // K, K × ndim
    DevBuf<int> bbox;                   // K × 2 × ndim
    hipStream_t stream = nullptr;
};

// returns 0, 1 (refused: *err says why) or 2 (a HIP call failed); stats is filled whenever the counters were read
int cc_build(const LsmHandle* h, CcWorkspace** workspace, double level, int side, const void* phi, CcObject** out, long long stats[4], const char** err) {
    const int ndim = h->grid.ndim;
    if (ndim != 2 && ndim != 3) { *err = "components: 2-D and 3-D fields only"; return 1; }
    const hipStream_t stream = h->stream;
    std::unique_ptr<CcObject> o(new CcObject());
    CcArgs& a = o->a;
    a.nnode = 1; a.ntile = 1;
    for (int d = 0; d < 3; ++d) {
        const int edge = ndim == 2 ? (d == 0 ? CcTile<2>::X : d == 1 ? CcTile<2>::Y : 1) : (d == 0 ? CcTile<3>::X : d == 1 ? CcTile<3>::Y : CcTile<3>::Z);
        a.n[d] = d < ndim ? h->nloc[d] : 1;
        if (a.n[d] < 1) { *err = "components: an empty grid"; return 1; }
        a.nt[d] = (a.n[d] + edge - 1) / edge;
        if (a.nnode > (long long)INT_MAX / a.n[d]) { *err = "components: the grid has 2^31 - 1 nodes or more"; return 1; }
        a.nnode *= a.n[d];
        a.ntile *= a.nt[d];
    }
    if (a.nnode >= (long long)INT_MAX) { *err = "components: the grid has 2^31 - 1 nodes or more"; return 1; }
    a.s1 = h->lay.stride[1]; a.s2 = ndim > 2 ? h->lay.stride[2] : 0; a.origin = h->lay.origin;
    a.nchunk = (a.nnode + CC_CHUNK - 1) / CC_CHUNK;
    if (a.ntile * 512 >= (1LL << 32)) { *err = "components: the grid has too many tiles for one launch"; return 1; }
    a.level = level; a.side = side; a.f32 = h->dtype == LSM_DTYPE_F32;
    o->ndim = ndim;
    o->stream = stream;

    if (!*workspace) *workspace = new CcWorkspace();     // the handle's, created by its first call; the buffers only grow
    CcWorkspace& W = **workspace;
    MOD_HIP(W.parent.grow((size_t)a.nnode * sizeof(unsigned)), "hipMalloc(parents)");
    MOD_HIP(W.sums.grow((size_t)a.nchunk * sizeof(unsigned)), "hipMalloc(chunk sums)");
    MOD_HIP(W.off.grow((size_t)a.nchunk * sizeof(unsigned)), "hipMalloc(chunk offsets)");
    MOD_HIP(W.st.grow((CC_NSTAT + 2) * sizeof(unsigned long long)), "hipMalloc(counters)");
    MOD_HIP(hipMemsetAsync(W.st.p, 0, (CC_NSTAT + 2) * sizeof(unsigned long long), stream), "components: memset");
    const unsigned tile_threads = ndim == 2 ? CcTile<2>::X * CcTile<2>::Y : CcTile<3>::X * CcTile<3>::Y * CcTile<3>::Z;
    const unsigned ntile = (unsigned)a.ntile, nchunk = (unsigned)a.nchunk;

    LSM_LAUNCH_ND(ndim, cc_local_kernel, ntile, tile_threads, stream, a, phi, W.parent.p, W.st.p);
    LSM_LAUNCH_ND(ndim, cc_merge_kernel, ntile, tile_threads, stream, a, W.parent.p, W.st.p);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(nchunk), dim3(256), 0, stream, a, W.parent.p, W.sums.p);
    chunk_scan<1, unsigned>(stream, {{{W.sums.p, W.off.p, 0}}}, a.nchunk, W.st.p + CC_K);
    MOD_HIP(hipGetLastError(), "components: launch failed");
    unsigned long long st[CC_NSTAT] = {};
    MOD_HIP(hipMemcpyAsync(st, W.st.p, sizeof(st), hipMemcpyDeviceToHost, stream), "components: counts");
    MOD_HIP(hipStreamSynchronize(stream), "components: device error");
    stats[0] = (long long)st[CC_K];
    stats[1] = (long long)st[CC_SET];
    stats[2] = (long long)st[CC_CROSS];
    stats[3] = (long long)st[CC_NONFINITE];
    if (st[CC_NONFINITE]) { *err = "components: phi must be finite"; return 1; }
    const long long K = o->K = (long long)st[CC_K];
    if (K > a.nnode) { *err = "components: more roots than nodes"; return 2; }

    MOD_HIP(o->labels.alloc((size_t)a.nnode * sizeof(int)), "hipMalloc(labels)");
    MOD_HIP(o->nodes.alloc((size_t)std::max(K, 1LL) * sizeof(long long)), "hipMalloc(component sizes)");
    MOD_HIP(o->sums.alloc((size_t)std::max(K, 1LL) * ndim * sizeof(long long)), "hipMalloc(index sums)");
    MOD_HIP(o->bbox.alloc((size_t)std::max(K, 1LL) * 2 * ndim * sizeof(int)), "hipMalloc(bounding boxes)");
    if (K) {
        hipLaunchKernelGGL(cc_init_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, K, ndim, o->nodes.p, o->sums.p, o->bbox.p);
        hipLaunchKernelGGL(cc_number_kernel, dim3(nchunk), dim3(256), 0, stream, a, (const unsigned*)W.parent.p, (const unsigned*)W.off.p, o->labels.p);
    }
    LSM_LAUNCH_ND(ndim, cc_label_kernel, ntile, tile_threads, stream, a, (const unsigned*)W.parent.p, o->labels.p, o->nodes.p, o->sums.p, o->bbox.p);
    MOD_HIP(hipGetLastError(), "components: launch failed");
    MOD_HIP(hipStreamSynchronize(stream), "components: device error");
    *out = o.release();
    return 0;
}

int cc_read(CcObject* o, int* labels, long long* nodes, long long* sums, int* bbox, const char** err) {
    const size_t K = (size_t)o->K, N = (size_t)o->ndim;
    return kuhn_read(o->stream, {{labels, o->labels, (size_t)o->a.nnode * sizeof(int)}, {nodes, o->nodes, K * sizeof(long long)},
                                 {sums, o->sums, K * N * sizeof(long long)}, {bbox, o->bbox, K * 2 * N * sizeof(int)}},
                     "components read: device error", err);
}

// returns 0, 1 (phi no longer matches the object: untouched) or 2 (a HIP call failed)
int cc_flip(CcObject* o, CcWorkspace* W, void* phi, const unsigned char* which, long long* flipped, const char** err) {
    const int ndim = o->ndim;
    const hipStream_t stream = o->stream;
    const CcArgs& a = o->a;
    *flipped = 0;
    if (!o->K) return 0;
    unsigned long long* cnt = W->st.p + CC_NSTAT;
    MOD_HIP(hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), stream), "components flip: memset");
    const unsigned nblk = (unsigned)((a.nnode + 255) / 256);
    LSM_LAUNCH_ND(ndim, cc_flip_count_kernel, nblk, 256, stream, a, (const void*)phi, (const int*)o->labels.p, which, cnt);
    unsigned long long c[2] = {};
    MOD_HIP(hipGetLastError(), "components flip: launch failed");
    MOD_HIP(hipMemcpyAsync(c, cnt, sizeof(c), hipMemcpyDeviceToHost, stream), "components flip: counts");
    MOD_HIP(hipStreamSynchronize(stream), "components flip: device error");
    if (c[CC_MISMATCH]) { *err = "components flip: phi has changed since the components were labelled (a flagged node is on the other side of level)"; return 1; }
    if (c[CC_FLAGGED]) {
        LSM_LAUNCH_ND(ndim, cc_flip_write_kernel, nblk, 256, stream, a, phi, (const int*)o->labels.p, which);
        MOD_HIP(hipGetLastError(), "components flip: launch failed");
        MOD_HIP(hipStreamSynchronize(stream), "components flip: device error");
    }
    *flipped = (long long)c[CC_FLAGGED];
    return 0;
}

void cc_free(CcObject* o) { delete o; }

}  // namespace lsm
