// lsm_iso.hip — isosurface(ϕ, level) on the device: the interface {ϕ = level} as an indexed mesh (segments in 2-D, triangles
// in 3-D), what ext/MMGSurfaceExt.jl:48-50 gets from marching cubes and ext/MakieExt.jl from contour!.  Marching simplices on
// the Freudenthal (Kuhn) subdivision of every cell: N! simplices per cell, one per permutation π of the axes in lexicographic
// order, with the corner chain m₀ = 0, m₁ = m₀ | 1<<π(0), …, m_N = 2^N − 1 (corner masks: bit a = axis a).  No ambiguous
// cases, a watertight and consistently oriented mesh of the zero set of the piecewise-linear interpolant, shared vertices
// (DESIGN.md §7.11).  tests/_iso_ref.py restates it; the rules:
//   * inside(I) := ϕ[I] < level (ϕ == level and NaN are outside); f32 storage widens exactly, all arithmetic is fp64;
//   * edge (I, d), d a non-empty mask, carries a vertex iff I + d is in the grid, inside(I) != inside(I + d) and an active cell
//     contains the edge (dense: every cell; band: the cells whose 2^N corners are band nodes — only band values decide);
//     vertices are numbered by ascending node (axis 0 fastest), then ascending d; the position is (lc + i·h) + t·h along the axes
//     of d, t = (level − ϕ_a)/(ϕ_b − ϕ_a) with a = I, b = I + d: one division per vertex;
//   * active cells ascending, simplices in permutation order: k inside corners, 0 < k < N + 1, give one segment (2-D), one
//     triangle (3-D, k = 1, 3) or two (k = 2); the orientation comes from a table over the sign pattern and the parity of π
//     (never a geometric test: degenerate elements get one too): normals point from inside to outside.
// Kernels: a classify sweep (one thread per node: a byte of edge mask and a byte of element count, sums per chunk of nodes),
// a scan of the chunk sums in one workgroup, an ordered compaction of the nodes that own a vertex or an element (with their
// vertex and element offsets; the vertex offset also goes into a node-indexed array that is written and read at those nodes
// only), and one thread per listed node for the vertices and for the elements.  No atomic decides an output position.
#include <algorithm>

#include "lsm_handle.h"

namespace lsm {

constexpr int ISO_CHUNK = 4096;            // nodes per workgroup of the classify and compaction kernels
constexpr int ISO_PER = ISO_CHUNK / 256;   // nodes per thread

struct IsoArgs {
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
constexpr int iso_nsimplex(int N) { return N == 2 ? 2 : 6; }
constexpr unsigned iso_chain(int N, int p) {
    return N == 2 ? (p == 0 ? 0310u : 0320u)
                  : (p == 0 ? 07310u : p == 1 ? 07510u : p == 2 ? 07320u : p == 3 ? 07620u : p == 4 ? 07540u : 07640u);
}
constexpr unsigned iso_odd(int N) { return N == 2 ? 0x2u : 0x26u; }
// elements per sign pattern on an even permutation: bits 0..1 the count, then 3 edge codes per triangle (3 bits each; 3-D) or
// 2 per segment (2 bits each; 2-D); an odd permutation swaps the last two vertices.  Edge codes: the pair (j, k) of chain
// positions in the order 01, 02, 03, 12, 13, 23 (3-D) or 01, 02, 12 (2-D).
__device__ const unsigned ISO_TET[16] = {0x0, 0x221, 0x381, 0x70c46, 0x565, 0xac2a2, 0x34582, 0x589,
                                         0x4a9, 0x94522, 0xa83a2, 0x3a5, 0x50c66, 0x461, 0x141, 0x0};
__device__ const unsigned ISO_SEG[8] = {0x0, 0x11, 0x9, 0x19, 0x25, 0x21, 0x5, 0x0};

template <int N>
__device__ __forceinline__ long long iso_off(const IsoArgs& a, int m) {     // padded offset of corner m
    return (m & 1) + ((m & 2) ? a.s1 : 0) + (N > 2 && (m & 4) ? a.s2 : 0);
}
template <int N>
__device__ __forceinline__ long long iso_lin_off(const IsoArgs& a, int m) { // the same in node numbers
    return (m & 1) + ((m & 2) ? (long long)a.n[0] : 0) + (N > 2 && (m & 4) ? (long long)a.n[0] * a.n[1] : 0);
}
template <int N>
__device__ __forceinline__ void iso_unlin(const IsoArgs& a, long long lin, int I[3]) {
    I[0] = (int)(lin % a.n[0]);
    const long long r = lin / a.n[0];
    I[1] = N > 2 ? (int)(r % a.n[1]) : (int)r;
    I[2] = N > 2 ? (int)(r / a.n[1]) : 0;
}
// corners of the cell anchored at I that are grid nodes: bit m of the result; up = the axes with I + 1 in the grid
template <int N>
__device__ __forceinline__ unsigned iso_up(const IsoArgs& a, const int I[3]) {
    return (I[0] + 1 < a.n[0] ? 1u : 0u) | (I[1] + 1 < a.n[1] ? 2u : 0u) | (N > 2 && I[2] + 1 < a.n[2] ? 4u : 0u);
}
// is the cell anchored at I − m' in the grid with all its corners on the band?
template <int N>
__device__ __forceinline__ bool iso_cell_active(const IsoArgs& a, const int I[3], int mp) {
    const int C[3] = {I[0] - (mp & 1), I[1] - ((mp >> 1) & 1), N > 2 ? I[2] - ((mp >> 2) & 1) : 0};
#pragma unroll
    for (int d = 0; d < N; ++d)
        if (C[d] < 0 || C[d] + 1 >= a.n[d]) return false;
    const long long q = a.origin + C[0] + C[1] * a.s1 + (N > 2 ? C[2] * a.s2 : 0);
    bool act = true;
    for (int m = 0; m < (1 << N); ++m) act = act && a.mask[q + iso_off<N>(a, m)] != 0;
    return act;
}
// elements of the cell whose corners have the inside flags `in` (bit m = corner m)
template <int N>
__device__ __forceinline__ unsigned iso_count(unsigned in) {
    unsigned c = 0;
#pragma unroll
    for (int p = 0; p < iso_nsimplex(N); ++p) {
        const unsigned ch = iso_chain(N, p);
        unsigned k = 0;
#pragma unroll
        for (int j = 0; j <= N; ++j) k += (in >> ((ch >> (3 * j)) & 7)) & 1;
        c += (k == 0 || k == N + 1) ? 0u : (N == 3 && k == 2 ? 2u : 1u);
    }
    return c;
}

// per node: the edges it owns that carry a vertex (bit d − 1) and the elements of the cell it anchors; per chunk the numbers of
// vertices, elements and nodes that own any.  Lane l + 1 holds node lin + 1: the x + 1 corners come from it by a shuffle.
template <int N>
__global__ void __launch_bounds__(256) iso_classify_kernel(IsoArgs a, unsigned char* emask, unsigned char* ecnt, unsigned* sums, long long nchunk) {
    __shared__ unsigned tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    const long long c0 = (long long)blockIdx.x * ISO_CHUNK;
    const int lane = threadIdx.x & 63;
    unsigned nv = 0, ne = 0, nl = 0;
    int I[3];
    iso_unlin<N>(a, c0 + threadIdx.x < a.nnode ? c0 + threadIdx.x : a.nnode - 1, I);
    for (int k = 0; k < ISO_PER; ++k) {
        const long long lin = c0 + threadIdx.x + 256 * k;
        const bool valid = lin < a.nnode;
        const unsigned up = valid ? iso_up<N>(a, I) : 0u;
        const long long q = a.origin + I[0] + I[1] * a.s1 + (N > 2 ? I[2] * a.s2 : 0);
        unsigned in = 0;       // inside flags of the corners that are grid nodes
#pragma unroll
        for (int m = 0; m < (1 << N); m += 2) {
            const bool have = valid && (m & ~up) == 0;
            const double v = have ? ld_val(a.phi, q + iso_off<N>(a, m), a.f32) : 0.0;
            double vx = __shfl_down(v, 1, 64);
            if (lane == 63 && (up & 1) && have) vx = ld_val(a.phi, q + iso_off<N>(a, m | 1), a.f32);
            if (have && v < a.level) in |= 1u << m;
            if (have && (up & 1) && vx < a.level) in |= 1u << (m | 1);
        }
        unsigned em = 0, ec = 0;
        if (valid) {
#pragma unroll
            for (int d = 1; d < (1 << N); ++d)
                if ((d & ~up) == 0 && ((in ^ (in >> d)) & 1)) em |= 1u << (d - 1);
            if (em && a.mask) {       // band: an edge needs an active cell around it
                unsigned act = 0;
                for (int mp = 0; mp < (1 << N); ++mp) act |= iso_cell_active<N>(a, I, mp) ? 1u << mp : 0u;
                unsigned keep = 0;
                for (int d = 1; d < (1 << N); ++d) {
                    bool cover = false;
                    for (int mp = 0; mp < (1 << N); ++mp) cover = cover || (!(mp & d) && ((act >> mp) & 1));
                    if (cover) keep |= 1u << (d - 1);
                }
                em &= keep;
                if (up == (1u << N) - 1 && (act & 1)) ec = iso_count<N>(in);
            } else if (em && up == (1u << N) - 1) {
                ec = iso_count<N>(in);
            }
        }
        emask[lin] = (unsigned char)em;     // the arrays cover whole chunks
        ecnt[lin] = (unsigned char)ec;
        nv += __popc(em);
        ne += ec;
        nl += (em | ec) != 0;
        // the thread's next node is 256 further: at most one wrap per axis on rows of 256 nodes or more, 256 / n[0] on tiny grids
        I[0] += 256;
        while (I[0] >= a.n[0]) { I[0] -= a.n[0]; ++I[1]; }
        if (N > 2)
            while (I[1] >= a.n[1]) { I[1] -= a.n[1]; ++I[2]; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        nv += __shfl_xor(nv, d, 64);
        ne += __shfl_xor(ne, d, 64);
        nl += __shfl_xor(nl, d, 64);
    }
    if (lane == 0) { atomicAdd(&tot[0], nv); atomicAdd(&tot[1], ne); atomicAdd(&tot[2], nl); }
    __syncthreads();
    if (threadIdx.x < 3) sums[threadIdx.x * nchunk + blockIdx.x] = tot[threadIdx.x];
}

// exclusive scans of the three rows of `in` (n values each) in one workgroup of 1024 threads, 8 consecutive values per thread per
// round; the totals into tot[0..2]
__global__ void __launch_bounds__(1024) iso_scan_kernel(const unsigned* in, long long n, long long* out, long long* tot) {
    __shared__ long long s[3][1024];
    long long carry[3] = {0, 0, 0};
    const int t = threadIdx.x;
    for (long long base = 0; base < n; base += 8 * 1024) {
        unsigned v[3][8];
        long long acc[3] = {0, 0, 0};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const long long i = base + 8LL * t + e;
                v[r][e] = i < n ? in[r * n + i] : 0u;
                acc[r] += v[r][e];
            }
#pragma unroll
        for (int r = 0; r < 3; ++r) s[r][t] = acc[r];
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {     // Hillis–Steele inclusive scan of the thread sums
            long long x[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) x[r] = t >= d ? s[r][t - d] : 0;
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 3; ++r) s[r][t] += x[r];
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            long long e0 = carry[r] + s[r][t] - acc[r];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const long long i = base + 8LL * t + e;
                if (i < n) out[r * n + i] = e0;
                e0 += v[r][e];
            }
            carry[r] += s[r][1023];
        }
        __syncthreads();
    }
    if (t < 3) tot[t] = carry[t];
}

// the nodes of every chunk that own a vertex or an element, ascending, at the chunk's scanned offset: node, vertex offset,
// element offset; vbase[node] := vertex offset where the node owns a vertex
__global__ void __launch_bounds__(256) iso_compact_kernel(const unsigned char* emask, const unsigned char* ecnt, long long nnode, const long long* off,
                                                          long long nchunk, long long* list, long long* list_v, long long* list_e, unsigned* vbase) {
    __shared__ unsigned s[3][256];
    const int t = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * ISO_CHUNK + (long long)t * ISO_PER;
    const uint4 em4 = *reinterpret_cast<const uint4*>(emask + c0), ec4 = *reinterpret_cast<const uint4*>(ecnt + c0);
    const unsigned emw[4] = {em4.x, em4.y, em4.z, em4.w}, ecw[4] = {ec4.x, ec4.y, ec4.z, ec4.w};
    unsigned m[3] = {0, 0, 0};
#pragma unroll
    for (int e = 0; e < ISO_PER; ++e) {
        const unsigned em = (emw[e / 4] >> (8 * (e % 4))) & 255u, ec = (ecw[e / 4] >> (8 * (e % 4))) & 255u;
        m[0] += __popc(em);
        m[1] += ec;
        m[2] += (em | ec) != 0;
    }
    for (int r = 0; r < 3; ++r) s[r][t] = m[r];
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        unsigned x[3];
        for (int r = 0; r < 3; ++r) x[r] = t >= d ? s[r][t - d] : 0;
        __syncthreads();
        for (int r = 0; r < 3; ++r) s[r][t] += x[r];
        __syncthreads();
    }
    long long pv = off[blockIdx.x] + s[0][t] - m[0], pe = off[nchunk + blockIdx.x] + s[1][t] - m[1],
              pl = off[2 * nchunk + blockIdx.x] + s[2][t] - m[2];
#pragma unroll
    for (int e = 0; e < ISO_PER; ++e) {
        const unsigned em = (emw[e / 4] >> (8 * (e % 4))) & 255u, ec = (ecw[e / 4] >> (8 * (e % 4))) & 255u;
        if (em | ec) {          // zero past the last node: the classify sweep writes whole chunks
            list[pl] = c0 + e;
            list_v[pl] = pv;
            list_e[pl] = pe;
            ++pl;
            if (em) vbase[c0 + e] = (unsigned)pv;
        }
        pv += __popc(em);
        pe += ec;
    }
}

// the vertices of the edges a listed node owns
template <int N>
__global__ void __launch_bounds__(256) iso_vertex_kernel(IsoArgs a, const unsigned char* emask, const long long* list, const long long* list_v,
                                                         long long nlist, double* verts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nlist) return;
    const long long lin = list[i];
    const unsigned em = emask[lin];
    if (!em) return;
    int I[3];
    iso_unlin<N>(a, lin, I);
    const long long q = a.origin + I[0] + I[1] * a.s1 + (N > 2 ? I[2] * a.s2 : 0);
    const double pa = ld_val(a.phi, q, a.f32);
    double x[3];
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = a.lc[e] + (double)I[e] * a.h[e];
    long long p = list_v[i];
#pragma unroll
    for (int d = 1; d < (1 << N); ++d) {
        if (!((em >> (d - 1)) & 1)) continue;
        const double pb = ld_val(a.phi, q + iso_off<N>(a, d), a.f32);
        const double t = (a.level - pa) / (pb - pa);
#pragma unroll
        for (int e = 0; e < N; ++e) verts[p * N + e] = ((d >> e) & 1) ? x[e] + t * a.h[e] : x[e];
        ++p;
    }
}

// the elements of the cell a listed node anchors
template <int N>
__global__ void __launch_bounds__(256) iso_element_kernel(IsoArgs a, const unsigned char* emask, const unsigned char* ecnt, const unsigned* vbase,
                                                          const long long* list, const long long* list_e, long long nlist, long long* elems) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nlist) return;
    const long long lin = list[i];
    if (!ecnt[lin]) return;
    int I[3];
    iso_unlin<N>(a, lin, I);
    const long long q = a.origin + I[0] + I[1] * a.s1 + (N > 2 ? I[2] * a.s2 : 0);
    unsigned in = 0;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) in |= ld_val(a.phi, q + iso_off<N>(a, m), a.f32) < a.level ? 1u << m : 0u;
    long long p = list_e[i];
#pragma unroll
    for (int sp = 0; sp < iso_nsimplex(N); ++sp) {
        const unsigned ch = iso_chain(N, sp);
        const bool odd = (iso_odd(N) >> sp) & 1;
        unsigned s = 0;
#pragma unroll
        for (int j = 0; j <= N; ++j) s |= ((in >> ((ch >> (3 * j)) & 7)) & 1) << j;
        const unsigned w = N == 3 ? ISO_TET[s] : ISO_SEG[s];
        const int cnt = w & 3;
        for (int t = 0; t < cnt; ++t) {
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const int cs = odd && c >= N - 2 ? (2 * N - 3) - c : c;      // an odd permutation swaps the last two vertices
                int j, k;
                if (N == 3) {
                    const unsigned code = (w >> (2 + 3 * (3 * t + cs))) & 7;
                    j = (0x940u >> (2 * code)) & 3;       // 01 02 03 12 13 23
                    k = (0xFB9u >> (2 * code)) & 3;
                } else {
                    const unsigned code = (w >> (2 + 2 * cs)) & 3;
                    j = (0x10u >> (2 * code)) & 3;        // 01 02 12
                    k = (0x29u >> (2 * code)) & 3;
                }
                const int mj = (ch >> (3 * j)) & 7, d = ((ch >> (3 * k)) & 7) ^ mj;
                const long long J = lin + iso_lin_off<N>(a, mj);
                elems[p * N + c] = (long long)vbase[J] + __popc(emask[J] & ((1u << (d - 1)) - 1u));
            }
            ++p;
        }
    }
}

// ---- host side
struct IsoObject {
    DevBuf<double> verts;
    DevBuf<long long> elems;
    long long nv = 0, ne = 0;
    int ndim = 0;
    hipStream_t stream = nullptr;
};

#define ISO_HIP(call, what) do { if ((call) != hipSuccess) { *err = what; delete o; return 2; } } while (0)

int iso_build(int ndim, const int n[3], long long s1, long long s2, long long origin, const double lc[3], const double h[3], double level,
              const void* phi, int f32, const unsigned char* mask, hipStream_t stream, IsoObject** out, long long counts_out[2], const char** err) {
    if (ndim != 2 && ndim != 3) { *err = "isosurface: 2-D and 3-D fields only"; return 1; }
    IsoArgs a;
    a.nnode = 1;
    for (int d = 0; d < 3; ++d) {
        a.n[d] = d < ndim ? n[d] : 1;
        a.lc[d] = d < ndim ? lc[d] : 0.0;
        a.h[d] = d < ndim ? h[d] : 1.0;
        if (d < ndim && n[d] < 2) { *err = "isosurface: at least two nodes per dimension"; return 1; }
        a.nnode *= a.n[d];
    }
    a.s1 = s1; a.s2 = ndim > 2 ? s2 : 0; a.origin = origin;
    a.level = level; a.phi = phi; a.f32 = f32; a.mask = mask;
    const long long nchunk = (a.nnode + ISO_CHUNK - 1) / ISO_CHUNK;
    if (nchunk > (1LL << 23)) { *err = "isosurface: the grid has too many nodes"; return 1; }     // 256 threads per chunk in one launch

    IsoObject* o = new IsoObject();
    o->ndim = ndim;
    o->stream = stream;
    DevBuf<unsigned char> emask, ecnt;     // whole chunks
    DevBuf<unsigned> sums, vbase;          // [vertices | elements | listed nodes] per chunk; vertex offset of a node that owns a vertex
    DevBuf<long long> off, tot, list, list_v, list_e;
    ISO_HIP(emask.alloc((size_t)nchunk * ISO_CHUNK), "hipMalloc(edge masks)");
    ISO_HIP(ecnt.alloc((size_t)nchunk * ISO_CHUNK), "hipMalloc(element counts)");
    ISO_HIP(sums.alloc(3 * (size_t)nchunk * sizeof(unsigned)), "hipMalloc(chunk sums)");
    ISO_HIP(off.alloc(3 * (size_t)nchunk * sizeof(long long)), "hipMalloc(chunk offsets)");
    ISO_HIP(tot.alloc(3 * sizeof(long long)), "hipMalloc(totals)");
    const unsigned gchunk = (unsigned)nchunk;
    if (ndim == 2) hipLaunchKernelGGL(iso_classify_kernel<2>, dim3(gchunk), dim3(256), 0, stream, a, emask.p, ecnt.p, sums.p, nchunk);
    else hipLaunchKernelGGL(iso_classify_kernel<3>, dim3(gchunk), dim3(256), 0, stream, a, emask.p, ecnt.p, sums.p, nchunk);
    hipLaunchKernelGGL(iso_scan_kernel, dim3(1), dim3(1024), 0, stream, sums.p, nchunk, off.p, tot.p);
    long long th[3] = {0, 0, 0};
    ISO_HIP(hipMemcpyAsync(th, tot, 3 * sizeof(long long), hipMemcpyDeviceToHost, stream), "isosurface: counts");
    ISO_HIP(hipStreamSynchronize(stream), "isosurface: counts");
    o->nv = th[0];
    o->ne = th[1];
    const long long nlist = th[2];
    if (o->nv > 0xffffffffLL) { *err = "isosurface: more than 2^32 vertices"; delete o; return 1; }
    if (nlist) {
        ISO_HIP(vbase.alloc((size_t)a.nnode * sizeof(unsigned)), "hipMalloc(vertex offsets)");
        ISO_HIP(list.alloc((size_t)nlist * sizeof(long long)), "hipMalloc(node list)");
        ISO_HIP(list_v.alloc((size_t)nlist * sizeof(long long)), "hipMalloc(node list)");
        ISO_HIP(list_e.alloc((size_t)nlist * sizeof(long long)), "hipMalloc(node list)");
        ISO_HIP(o->verts.alloc((size_t)std::max(o->nv, 1LL) * ndim * sizeof(double)), "hipMalloc(vertices)");
        ISO_HIP(o->elems.alloc((size_t)std::max(o->ne, 1LL) * ndim * sizeof(long long)), "hipMalloc(elements)");
        hipLaunchKernelGGL(iso_compact_kernel, dim3(gchunk), dim3(256), 0, stream, emask.p, ecnt.p, a.nnode, off.p, nchunk, list.p, list_v.p, list_e.p,
                           vbase.p);
        const unsigned glist = (unsigned)((nlist + 255) / 256);
        if (ndim == 2) {
            hipLaunchKernelGGL(iso_vertex_kernel<2>, dim3(glist), dim3(256), 0, stream, a, emask.p, list.p, list_v.p, nlist, o->verts.p);
            hipLaunchKernelGGL(iso_element_kernel<2>, dim3(glist), dim3(256), 0, stream, a, emask.p, ecnt.p, vbase.p, list.p, list_e.p, nlist, o->elems.p);
        } else {
            hipLaunchKernelGGL(iso_vertex_kernel<3>, dim3(glist), dim3(256), 0, stream, a, emask.p, list.p, list_v.p, nlist, o->verts.p);
            hipLaunchKernelGGL(iso_element_kernel<3>, dim3(glist), dim3(256), 0, stream, a, emask.p, ecnt.p, vbase.p, list.p, list_e.p, nlist, o->elems.p);
        }
    }
    ISO_HIP(hipGetLastError(), "isosurface: launch failed");
    ISO_HIP(hipStreamSynchronize(stream), "isosurface: device error");     // the work buffers are released on return
    counts_out[0] = o->nv;
    counts_out[1] = o->ne;
    *out = o;
    return 0;
}
#undef ISO_HIP

int iso_read(IsoObject* o, double* verts, long long* elems, const char** err) {
    hipError_t e = hipSuccess;
    if (verts && o->nv) e = hipMemcpyAsync(verts, o->verts, (size_t)o->nv * o->ndim * sizeof(double), hipMemcpyDeviceToDevice, o->stream);
    if (elems && o->ne && e == hipSuccess)
        e = hipMemcpyAsync(elems, o->elems, (size_t)o->ne * o->ndim * sizeof(long long), hipMemcpyDeviceToDevice, o->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) { *err = "isosurface read: device error"; return 2; }
    return 0;
}

void iso_free(IsoObject* o) { delete o; }

}  // namespace lsm
