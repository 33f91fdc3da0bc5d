// kuhn.h — marching simplices on the Freudenthal (Kuhn) subdivision of every cell, the core that isosurface (lsm_iso.hip) and
// volume_mesh (lsm_vol.hip) share: N! simplices per cell, one per permutation π of the axes in lexicographic order, with the
// corner chain m₀ = 0, m₁ = m₀ | 1<<π(0), …, m_N = 2^N − 1 (corner masks: bit a = axis a).  No ambiguous cases, and the diagonals
// of neighbouring cells are translates of each other.  tests/_iso_ref.py restates the rules:
//   * inside(I) := ϕ[I] < level (ϕ == level and NaN are outside); f32 storage widens exactly, all arithmetic is fp64;
//   * edge (I, d), d a non-empty mask, carries a cut vertex iff I + d is in the grid and inside(I) != inside(I + d); node I owns
//     the cut vertices of its edges by ascending d; the position is (lc + i·h) + t·h along the axes of d,
//     t = (level − ϕ_a)/(ϕ_b − ϕ_a) with a = I, b = I + d: one division per vertex, no contraction (-ffp-contract=off);
//   * interface elements: cells ascending, simplices in permutation order: k inside corners, 0 < k < N + 1, give one segment
//     (2-D), one triangle (3-D, k = 1, 3) or two (k = 2); the orientation comes from a table over the sign pattern and the
//     parity of π (never a geometric test: degenerate elements get one too): normals point from inside to outside.
// Both features run a classify sweep (one thread per node: a byte of edge mask and a byte of element count, three sums per chunk
// of nodes), scan the chunk sums in one workgroup and read the three totals on the host; what follows is their own.
#pragma once
#include <initializer_list>

#include "lsm_handle.h"
#include "wave.h"

namespace lsm {

constexpr int KUHN_CHUNK = 4096;             // nodes per workgroup of the classify sweep and of the kernels that follow its chunks
constexpr int KUHN_PER = KUHN_CHUNK / 256;   // nodes per thread

struct KuhnArgs {
    int n[3];
    long long s1, s2, origin;   // the padded layout of ϕ and of the band mask
    long long nnode;
    double lc[3], h[3];
    double level;
    const void* phi;
    int f32;
    const unsigned char* mask;  // narrow band: 1 = band node (NULL = dense)
};

// the corner chain of simplex p, 3 bits per corner, and the parity of its permutation (bit p of the ODD mask)
constexpr int kuhn_nsimplex(int N) { return N == 2 ? 2 : 6; }
constexpr unsigned kuhn_chain(int N, int p) {
    return N == 2 ? (p == 0 ? 0310u : 0320u)
                  : (p == 0 ? 07310u : p == 1 ? 07510u : p == 2 ? 07320u : p == 3 ? 07620u : p == 4 ? 07540u : 07640u);
}
constexpr unsigned kuhn_odd(int N) { return N == 2 ? 0x2u : 0x26u; }
// interface elements per sign pattern on an even permutation: bits 0..1 the count, then 3 edge codes per triangle (3 bits each;
// 3-D) or 2 per segment (2 bits each; 2-D); an odd permutation swaps the last two vertices.  One definition in the source;
// `static`, so each of the two translation units that include this header carries its own device copy of these 24 words.
static __device__ const unsigned KUHN_TET[16] = {0x0, 0x221, 0x381, 0x70c46, 0x565, 0xac2a2, 0x34582, 0x589,
                                                 0x4a9, 0x94522, 0xa83a2, 0x3a5, 0x50c66, 0x461, 0x141, 0x0};
static __device__ const unsigned KUHN_SEG[8] = {0x0, 0x11, 0x9, 0x19, 0x25, 0x21, 0x5, 0x0};
// an edge code is the pair (j, k) of chain positions in the order 01, 02, 03, 12, 13, 23 (3-D) or 01, 02, 12 (2-D)
template <int N>
__device__ __forceinline__ void kuhn_edge(unsigned code, int& j, int& k) {
    j = ((N == 3 ? 0x940u : 0x10u) >> (2 * code)) & 3;
    k = ((N == 3 ? 0xFB9u : 0x29u) >> (2 * code)) & 3;
}
// the sign pattern of the simplex with chain ch: bit j = chain corner j inside (`in`: bit m = corner m of the cell)
template <int N>
__device__ __forceinline__ unsigned kuhn_pattern(unsigned in, unsigned ch) {
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j <= N; ++j) s |= ((in >> ((ch >> (3 * j)) & 7)) & 1) << j;
    return s;
}

template <int N>
__device__ __forceinline__ long long kuhn_off(const KuhnArgs& a, int m) {     // padded offset of corner m
    return (m & 1) + ((m & 2) ? a.s1 : 0) + (N > 2 && (m & 4) ? a.s2 : 0);
}
template <int N>
__device__ __forceinline__ long long kuhn_lin_off(const KuhnArgs& a, int m) { // the same in node numbers
    return (m & 1) + ((m & 2) ? (long long)a.n[0] : 0) + (N > 2 && (m & 4) ? (long long)a.n[0] * a.n[1] : 0);
}
template <int N>
__device__ __forceinline__ void kuhn_unlin(const KuhnArgs& a, long long lin, int I[3]) {
    I[0] = (int)(lin % a.n[0]);
    const long long r = lin / a.n[0];
    I[1] = N > 2 ? (int)(r % a.n[1]) : (int)r;
    I[2] = N > 2 ? (int)(r / a.n[1]) : 0;
}
template <int N>
__device__ __forceinline__ long long kuhn_node(const KuhnArgs& a, const int I[3]) {   // padded index of node I
    return a.origin + I[0] + I[1] * a.s1 + (N > 2 ? I[2] * a.s2 : 0);
}
// the axes with I + 1 in the grid: corner m of the cell anchored at I is a grid node iff (m & ~up) == 0
template <int N>
__device__ __forceinline__ unsigned kuhn_up(const KuhnArgs& a, const int I[3]) {
    return (I[0] + 1 < a.n[0] ? 1u : 0u) | (I[1] + 1 < a.n[1] ? 2u : 0u) | (N > 2 && I[2] + 1 < a.n[2] ? 4u : 0u);
}

// ---- the classify sweep: a workgroup of 256 threads takes a chunk, thread t the nodes c0 + t + 256·k of it, k < KUHN_PER; it
// starts at kuhn_unlin of its first node (clamped to the last node of the grid) and walks on with kuhn_advance

// inside flags of the corners of the cell anchored at the thread's node I (padded index q) that are grid nodes: bit m = corner m.
// Lane l + 1 holds node lin + 1: the x + 1 corners come from it by a shuffle, lane 63 loads its own.  `up` is 0 past the last
// node.  Every lane of the wave calls this.
template <int N>
__device__ __forceinline__ unsigned kuhn_inside(const KuhnArgs& a, long long q, unsigned up, bool valid) {
    const int lane = threadIdx.x & 63;
    unsigned in = 0;
#pragma unroll
    for (int m = 0; m < (1 << N); m += 2) {
        const bool have = valid && (m & ~up) == 0;
        const double v = have ? ld_val(a.phi, q + kuhn_off<N>(a, m), a.f32) : 0.0;
        double vx = __shfl_down(v, 1, 64);
        if (lane == 63 && (up & 1) && have) vx = ld_val(a.phi, q + kuhn_off<N>(a, m | 1), a.f32);
        if (have && v < a.level) in |= 1u << m;
        if (have && (up & 1) && vx < a.level) in |= 1u << (m | 1);
    }
    return in;
}
// the edges (I, d) in the grid that change sign: bit d − 1
template <int N>
__device__ __forceinline__ unsigned kuhn_edges(unsigned in, unsigned up) {
    unsigned em = 0;
#pragma unroll
    for (int d = 1; d < (1 << N); ++d)
        if ((d & ~up) == 0 && ((in ^ (in >> d)) & 1)) em |= 1u << (d - 1);
    return em;
}
// the thread's next node is 256 further: at most one wrap per axis on rows of 256 nodes or more, 256 / n[0] on tiny grids
template <int N>
__device__ __forceinline__ void kuhn_advance(const KuhnArgs& a, int I[3]) {
    I[0] += 256;
    while (I[0] >= a.n[0]) { I[0] -= a.n[0]; ++I[1]; }
    if (N > 2)
        while (I[1] >= a.n[1]) { I[1] -= a.n[1]; ++I[2]; }
}
// sums[r·nchunk + chunk] := the workgroup's sum of x_r, r < 3 (integer sums: any order gives the same).  Every thread calls this.
__device__ __forceinline__ void kuhn_chunk_sums(unsigned x0, unsigned x1, unsigned x2, unsigned* sums, long long nchunk) {
    __shared__ unsigned wsum[3][4];
    x0 = block_sum<4>(x0, wsum[0]); x1 = block_sum<4>(x1, wsum[1]); x2 = block_sum<4>(x2, wsum[2]);
    if (threadIdx.x == 0) { sums[blockIdx.x] = x0; sums[nchunk + blockIdx.x] = x1; sums[2 * nchunk + blockIdx.x] = x2; }
}

// ---- what the later kernels share

// the cut vertices of the edges in `em` (bit d − 1) of the node at x (padded index q) into verts[p], verts[p + 1], …
template <int N>
__device__ __forceinline__ void kuhn_cut_vertices(const KuhnArgs& a, long long q, const double x[3], unsigned em, long long p, double* verts) {
    const double pa = ld_val(a.phi, q, a.f32);
#pragma unroll
    for (int d = 1; d < (1 << N); ++d) {
        if (!((em >> (d - 1)) & 1)) continue;
        const double pb = ld_val(a.phi, q + kuhn_off<N>(a, d), a.f32);
        const double t = (a.level - pa) / (pb - pa);
#pragma unroll
        for (int e = 0; e < N; ++e) verts[p * N + e] = ((d >> e) & 1) ? x[e] + t * a.h[e] : x[e];
        ++p;
    }
}
// the interface elements of the cell anchored at node lin, whose corners have the inside flags `in`, into out[p], out[p + 1], …;
// vertex_id(J, d) is the number of the cut vertex on edge (J, d)
template <int N, class VertexId>
__device__ __forceinline__ void kuhn_interface_elements(const KuhnArgs& a, long long* out, long long lin, unsigned in, long long p,
                                                        VertexId vertex_id) {
#pragma unroll
    for (int sp = 0; sp < kuhn_nsimplex(N); ++sp) {
        const unsigned ch = kuhn_chain(N, sp);
        const bool odd = (kuhn_odd(N) >> sp) & 1;
        const unsigned w = N == 3 ? KUHN_TET[kuhn_pattern<N>(in, ch)] : KUHN_SEG[kuhn_pattern<N>(in, ch)];
        const int cnt = w & 3;
        for (int t = 0; t < cnt; ++t) {
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const int cs = odd && c >= N - 2 ? (2 * N - 3) - c : c;      // an odd permutation swaps the last two vertices
                int j, k;
                kuhn_edge<N>(N == 3 ? (w >> (2 + 3 * (3 * t + cs))) & 7 : (w >> (2 + 2 * cs)) & 3, j, k);
                const int mj = (ch >> (3 * j)) & 7, d = ((ch >> (3 * k)) & 7) ^ mj;
                out[p * N + c] = vertex_id(lin + kuhn_lin_off<N>(a, mj), d);
            }
            ++p;
        }
    }
}

// ---- host side (defined in lsm_iso.hip)

// the front half of a build: kuhn_begin, the feature's classify sweep over w.nchunk chunks, kuhn_totals.  The buffers are
// released with the struct.
struct KuhnWork {
    KuhnArgs a;
    long long nchunk = 0;
    DevBuf<unsigned char> emask, ecnt;     // per node, whole chunks
    DevBuf<unsigned> sums;                 // three rows of chunk sums
    DevBuf<long long> off, tot;            // their exclusive scans; the three totals
    long long total[3] = {0, 0, 0};        // the totals on the host; total[0] is the number of vertices
};
// Both return 0, or 1 (refused) / 2 (device error) with *err set; msg holds the feature's refusals: not 2-D or 3-D, fewer than
// two nodes along an axis, more than max_chunks chunks, the read of the totals failed, more than 2^32 vertices.
// kuhn_begin fills w.a from the handle's grid and allocates the buffers.
int kuhn_begin(const LsmHandle* h, double level, const void* phi, const unsigned char* mask, long long max_chunks, const char* const msg[5],
               KuhnWork& w, const char** err);
// kuhn_totals scans the three rows of w.sums into w.off (scan.h's kernel, one workgroup) and reads the totals.
int kuhn_totals(KuhnWork& w, hipStream_t stream, const char* const msg[5], const char** err);
// device-to-device copies of the arrays the caller asked for (dst NULL or no bytes: skipped), then a synchronise
struct KuhnCopy { void* dst; const void* src; size_t bytes; };
int kuhn_read(hipStream_t stream, std::initializer_list<KuhnCopy> copies, const char* what, const char** err);

}  // namespace lsm
