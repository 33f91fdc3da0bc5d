// lsm_vol.hip — volume_mesh(ϕ, level) on the device: the body-fitted simplicial mesh of the interior {ϕ < level} (triangles in
// 2-D, tetrahedra in 3-D) whose boundary inside the box is isosurface's mesh — the splitting phase of mmg2d_O3 / mmg3d_O3 -ls that
// ext/MMGVolumeExt.jl (export_volume_mesh) runs over the Kuhn triangulation of the grid, without the remesher.
// The subdivision, the sign convention and the cut vertices are those of lsm_iso.hip (§7.11); tests/_vol_ref.py restates the rules:
//   * node I (ascending, axis 0 fastest) owns itself if ϕ[I] < level, at lc + i·h, then the cut vertices of its edges (I, d) by
//     ascending direction mask d, at (lc + i·h) + t·h, t = (level − ϕ_a)/(ϕ_b − ϕ_a): one division per vertex, no contraction;
//   * cells ascending, simplices in permutation order; with a < b < … the inside and c < d the outside corners by chain position
//     a simplex gives itself (all inside), nothing (none), (a, ac, ad) or (a, b, bc), (a, bc, ac) in 2-D, (a, ab', ac', ad'), the
//     prism u = (a, ac, ad), w = (b, bc, bd) or the prism u = (a, b, c), w = (ad, bd, cd) in 3-D, a prism being cut as
//     (u0, u1, u2, w2), (u0, u1, w1, w2), (u0, w0, w1, w2): no Steiner point, neighbours pick the same diagonals, the interface
//     quad is cut as isosurface cuts it;
//   * the last two vertices of an element are swapped by a table over (sign pattern, sub-element) xor the parity of π (never a
//     geometric test): every signed volume is >= 0;
//   * the interface elements are isosurface's, in its order and orientation, in this mesh's vertex numbering.
// Kernels: a classify sweep (one thread per node: a byte of edge mask with the inside bit, a byte of element count, a byte of
// interface count, sums per chunk of nodes), a scan of the chunk sums in one workgroup, the vertex offset of every node (a scan
// inside the chunk on top of the chunk's base), one thread per node for the vertices, and one workgroup per chunk for the
// elements: it scans the counts of 256 cells at a time, stages their elements in LDS as 32-bit vertex numbers and writes the
// stage out as one contiguous run of int64, 16 bytes per lane.  No atomic decides an output position.
#include <algorithm>

#include "lsm_handle.h"

namespace lsm {

constexpr int VOL_CHUNK = 4096;            // nodes per workgroup of the classify, offset and element kernels
constexpr int VOL_PER = VOL_CHUNK / 256;   // nodes per thread
constexpr int VOL_CAP = 2048;              // elements the LDS stage holds: 256 interior cells of 6 tetrahedra fit in one round

struct VolArgs {
    int n[3];
    long long s1, s2, origin;   // the padded layout of ϕ
    long long nnode;
    double lc[3], h[3];
    double level;
    const void* phi;
    int f32;
};

// the corner chain of simplex p, 3 bits per corner, and the parity of its permutation (bit p of the ODD mask): lsm_iso.hip's
constexpr int vol_nsimplex(int N) { return N == 2 ? 2 : 6; }
constexpr unsigned vol_chain(int N, int p) {
    return N == 2 ? (p == 0 ? 0310u : 0320u)
                  : (p == 0 ? 07310u : p == 1 ? 07510u : p == 2 ? 07320u : p == 3 ? 07620u : p == 4 ? 07540u : 07640u);
}
constexpr unsigned vol_odd(int N) { return N == 2 ? 0x2u : 0x26u; }
// sub-elements per sign pattern (bit j = chain corner j inside) on an even permutation, the orientation table applied: bits 0..1 the
// count, then N + 1 vertex codes per sub-element; an odd permutation swaps the last two vertices.  3-D codes, 4 bits: 0..3 the
// chain corner, 4 + the edge (j, k) in the order 01, 02, 03, 12, 13, 23.  2-D codes, 3 bits: 0..2 the corner, 3 + the edge in the
// order 01, 02, 12.
__device__ const unsigned long long VOL_TET[16] = {
    0x0ull, 0x19501ull, 0x1e105ull, 0x21c41e1421943ull, 0x25d49ull, 0x1e4825d01a503ull, 0x2548565066107ull, 0x2618224424843ull,
    0x2258dull, 0x260c225025503ull, 0x1a4c65905e507ull, 0x1e5425c40e443ull, 0x218c9a14a1d4bull, 0x21d01e0820c83ull, 0x159059484d887ull,
    0xc841ull};
__device__ const unsigned VOL_TRI[8] = {0x0u, 0x461u, 0x3a5u, 0x94522u, 0x589u, 0xac2a2u, 0x70c46u, 0x221u};
// the interface elements per sign pattern: lsm_iso.hip's tables (count in bits 0..1, then edge codes, 3 bits each in 3-D, 2 in 2-D)
__device__ const unsigned VOL_ISO_TET[16] = {0x0, 0x221, 0x381, 0x70c46, 0x565, 0xac2a2, 0x34582, 0x589,
                                             0x4a9, 0x94522, 0xa83a2, 0x3a5, 0x50c66, 0x461, 0x141, 0x0};
__device__ const unsigned VOL_ISO_SEG[8] = {0x0, 0x11, 0x9, 0x19, 0x25, 0x21, 0x5, 0x0};

template <int N>
__device__ __forceinline__ long long vol_off(const VolArgs& a, int m) {     // padded offset of corner m
    return (m & 1) + ((m & 2) ? a.s1 : 0) + (N > 2 && (m & 4) ? a.s2 : 0);
}
template <int N>
__device__ __forceinline__ long long vol_lin_off(const VolArgs& a, int m) { // the same in node numbers
    return (m & 1) + ((m & 2) ? (long long)a.n[0] : 0) + (N > 2 && (m & 4) ? (long long)a.n[0] * a.n[1] : 0);
}
template <int N>
__device__ __forceinline__ void vol_unlin(const VolArgs& a, long long lin, int I[3]) {
    I[0] = (int)(lin % a.n[0]);
    const long long r = lin / a.n[0];
    I[1] = N > 2 ? (int)(r % a.n[1]) : (int)r;
    I[2] = N > 2 ? (int)(r / a.n[1]) : 0;
}
// elements and interface elements of the cell whose corners have the inside flags `in` (bit m = corner m): bits 0..7 and 8..15
template <int N>
__device__ __forceinline__ unsigned vol_count(unsigned in) {
    unsigned c = 0;
#pragma unroll
    for (int p = 0; p < vol_nsimplex(N); ++p) {
        const unsigned ch = vol_chain(N, p);
        unsigned k = 0;
#pragma unroll
        for (int j = 0; j <= N; ++j) k += (in >> ((ch >> (3 * j)) & 7)) & 1;
        // 3-D: 0 1 3 3 1 elements and 0 1 2 1 0 triangles for k = 0..4; 2-D: 0 1 2 1 and 0 1 1 0
        c += N == 3 ? ((0x13310u >> (4 * k)) & 15) | (((0x01210u >> (4 * k)) & 15) << 8) : ((0x1210u >> (4 * k)) & 15) | (((0x0110u >> (4 * k)) & 15) << 8);
    }
    return c;
}
// the vertex number of the cut vertex on edge (J, d) from J's offset and mask byte
__device__ __forceinline__ unsigned vol_cut_id(unsigned vb, unsigned em, int d) { return vb + (em >> 7) + __popc(em & ((1u << (d - 1)) - 1u)); }

// per node: the edges it owns that carry a vertex (bit d − 1) and whether it is inside (bit 7), the elements and the interface
// elements of the cell it anchors; per chunk the numbers of vertices, elements and interface elements.  Lane l + 1 holds node
// lin + 1: the x + 1 corners come from it by a shuffle.
template <int N>
__global__ void __launch_bounds__(256) vol_classify_kernel(VolArgs a, unsigned char* emask, unsigned char* ecnt, unsigned char* icnt, unsigned* sums,
                                                           long long nchunk) {
    __shared__ unsigned tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    const long long c0 = (long long)blockIdx.x * VOL_CHUNK;
    const int lane = threadIdx.x & 63;
    unsigned nv = 0, ne = 0, ni = 0;
    int I[3];
    vol_unlin<N>(a, c0 + threadIdx.x < a.nnode ? c0 + threadIdx.x : a.nnode - 1, I);
    for (int k = 0; k < VOL_PER; ++k) {
        const long long lin = c0 + threadIdx.x + 256 * k;
        const bool valid = lin < a.nnode;
        const unsigned up = !valid ? 0u : (I[0] + 1 < a.n[0] ? 1u : 0u) | (I[1] + 1 < a.n[1] ? 2u : 0u) | (N > 2 && I[2] + 1 < a.n[2] ? 4u : 0u);
        const long long q = a.origin + I[0] + I[1] * a.s1 + (N > 2 ? I[2] * a.s2 : 0);
        unsigned in = 0;       // inside flags of the corners that are grid nodes
#pragma unroll
        for (int m = 0; m < (1 << N); m += 2) {
            const bool have = valid && (m & ~up) == 0;
            const double v = have ? ld_val(a.phi, q + vol_off<N>(a, m), a.f32) : 0.0;
            double vx = __shfl_down(v, 1, 64);
            if (lane == 63 && (up & 1) && have) vx = ld_val(a.phi, q + vol_off<N>(a, m | 1), a.f32);
            if (have && v < a.level) in |= 1u << m;
            if (have && (up & 1) && vx < a.level) in |= 1u << (m | 1);
        }
        unsigned em = 0, ec = 0, ic = 0;
        if (valid) {
#pragma unroll
            for (int d = 1; d < (1 << N); ++d)
                if ((d & ~up) == 0 && ((in ^ (in >> d)) & 1)) em |= 1u << (d - 1);
            if (up == (1u << N) - 1) {
                if (em) {
                    const unsigned c = vol_count<N>(in);
                    ec = c & 255u;
                    ic = c >> 8;
                } else if (in & 1) {
                    ec = vol_nsimplex(N);       // every corner inside
                }
            }
            em |= (in & 1) << 7;
        }
        emask[lin] = (unsigned char)em;     // the arrays cover whole chunks
        ecnt[lin] = (unsigned char)ec;
        icnt[lin] = (unsigned char)ic;
        nv += __popc(em);
        ne += ec;
        ni += ic;
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
        ni += __shfl_xor(ni, d, 64);
    }
    if (lane == 0) { atomicAdd(&tot[0], nv); atomicAdd(&tot[1], ne); atomicAdd(&tot[2], ni); }    // integer sums: any order gives the same
    __syncthreads();
    if (threadIdx.x < 3) sums[threadIdx.x * nchunk + blockIdx.x] = tot[threadIdx.x];
}

// exclusive scans of the three rows of `in` (n values each) in one workgroup of 1024 threads, 8 consecutive values per thread per
// round; the totals into tot[0..2]
__global__ void __launch_bounds__(1024) vol_scan_kernel(const unsigned* in, long long n, long long* out, long long* tot) {
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

// vbase[node] := the number of the first vertex the node owns: the chunk's scanned base plus a scan inside the chunk.  A thread
// takes VOL_PER consecutive nodes; the arrays cover whole chunks.
__global__ void __launch_bounds__(256) vol_offset_kernel(const unsigned char* emask, const long long* off, unsigned* vbase) {
    __shared__ unsigned wsum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long c0 = (long long)blockIdx.x * VOL_CHUNK + (long long)t * VOL_PER;
    const uint4 em4 = *reinterpret_cast<const uint4*>(emask + c0);
    const unsigned emw[4] = {em4.x, em4.y, em4.z, em4.w};
    unsigned m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) m += __popc(emw[w]);
    unsigned incl = m;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned p = (unsigned)off[blockIdx.x] + incl - m;
    for (int w = 0; w < wave; ++w) p += wsum[w];
    unsigned o[VOL_PER];
#pragma unroll
    for (int e = 0; e < VOL_PER; ++e) {
        o[e] = p;
        p += __popc((emw[e / 4] >> (8 * (e % 4))) & 255u);
    }
#pragma unroll
    for (int e = 0; e < VOL_PER; e += 4) *reinterpret_cast<uint4*>(vbase + c0 + e) = make_uint4(o[e], o[e + 1], o[e + 2], o[e + 3]);
}

// the vertices a node owns: itself if inside, then the cut vertices of its edges
template <int N>
__global__ void __launch_bounds__(256) vol_vertex_kernel(VolArgs a, const unsigned char* emask, const unsigned* vbase, double* verts) {
    const long long lin = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lin >= a.nnode) return;
    const unsigned em = emask[lin];
    if (!em) return;
    int I[3];
    vol_unlin<N>(a, lin, I);
    double x[3];
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = a.lc[e] + (double)I[e] * a.h[e];
    long long p = vbase[lin];
    if (em & 128u) {
#pragma unroll
        for (int e = 0; e < N; ++e) verts[p * N + e] = x[e];
        ++p;
    }
    if (!(em & 127u)) return;
    const long long q = a.origin + I[0] + I[1] * a.s1 + (N > 2 ? I[2] * a.s2 : 0);
    const double pa = ld_val(a.phi, q, a.f32);
#pragma unroll
    for (int d = 1; d < (1 << N); ++d) {
        if (!((em >> (d - 1)) & 1)) continue;
        const double pb = ld_val(a.phi, q + vol_off<N>(a, d), a.f32);
        const double t = (a.level - pa) / (pb - pa);
#pragma unroll
        for (int e = 0; e < N; ++e) verts[p * N + e] = ((d >> e) & 1) ? x[e] + t * a.h[e] : x[e];
        ++p;
    }
}

// the elements and the interface elements of a chunk's cells.  256 cells per pass: their counts are scanned in the workgroup, every
// thread puts the elements of its cell into the LDS stage at their place (32-bit vertex numbers), and the workgroup writes the
// stage to the pass's contiguous run of the output, consecutive lanes to consecutive addresses.  A pass with more than VOL_CAP
// elements (cut cells give up to 18) takes several rounds over windows of VOL_CAP elements.  The interface elements, a surface's
// worth, are written by their threads directly.
template <int N>
__global__ void __launch_bounds__(256) vol_element_kernel(VolArgs a, const unsigned char* emask, const unsigned char* ecnt, const unsigned char* icnt,
                                                          const unsigned* vbase, const long long* off, long long nchunk, long long* elems,
                                                          long long* iface) {
    constexpr int W = N + 1;
    __shared__ __attribute__((aligned(16))) unsigned stage[VOL_CAP * W];
    __shared__ unsigned wsum[2][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long c0 = (long long)blockIdx.x * VOL_CHUNK;
    long long ebase = off[nchunk + blockIdx.x], ibase = off[2 * nchunk + blockIdx.x];
    for (int k = 0; k < VOL_PER; ++k) {
        const long long lin = c0 + t + 256 * k;          // the count arrays cover whole chunks, zero past the last node
        const unsigned ec = ecnt[lin], ic = icnt[lin];
        const unsigned x = ec | (ic << 16);              // at most 256·18 and 256·12 per pass: two 16-bit sums in one word
        unsigned incl = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wsum[k & 1][wave] = incl;
        __syncthreads();
        unsigned excl = incl - x, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned s = wsum[k & 1][w];
            if (w < wave) excl += s;
            total += s;
        }
        const unsigned eoff = excl & 0xffffu, ioff = excl >> 16, etot = total & 0xffffu, itot = total >> 16;
        if (!etot) continue;                             // uniform; no elements, no interface
        const bool full = ec == (unsigned)vol_nsimplex(N) && ic == 0;      // no simplex is cut and all are kept: every corner inside
        unsigned in = 0;
        if (ec && !full) {
#pragma unroll
            for (int m = 0; m < (1 << N); ++m) in |= (unsigned)(emask[lin + vol_lin_off<N>(a, m)] >> 7) << m;
        }
        if (ic) {
            long long p = ibase + ioff;
#pragma unroll
            for (int sp = 0; sp < vol_nsimplex(N); ++sp) {
                const unsigned ch = vol_chain(N, sp);
                const bool odd = (vol_odd(N) >> sp) & 1;
                unsigned s = 0;
#pragma unroll
                for (int j = 0; j <= N; ++j) s |= ((in >> ((ch >> (3 * j)) & 7)) & 1) << j;
                const unsigned w = N == 3 ? VOL_ISO_TET[s] : VOL_ISO_SEG[s];
                const int cnt = w & 3;
                for (int e = 0; e < cnt; ++e) {
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        const int cs = odd && c >= N - 2 ? (2 * N - 3) - c : c;
                        int j, kk;
                        if (N == 3) {
                            const unsigned code = (w >> (2 + 3 * (3 * e + cs))) & 7;
                            j = (0x940u >> (2 * code)) & 3;       // 01 02 03 12 13 23
                            kk = (0xFB9u >> (2 * code)) & 3;
                        } else {
                            const unsigned code = (w >> (2 + 2 * cs)) & 3;
                            j = (0x10u >> (2 * code)) & 3;        // 01 02 12
                            kk = (0x29u >> (2 * code)) & 3;
                        }
                        const int mj = (ch >> (3 * j)) & 7, d = ((ch >> (3 * kk)) & 7) ^ mj;
                        const long long J = lin + vol_lin_off<N>(a, mj);
                        iface[p * N + c] = (long long)vol_cut_id(vbase[J], emask[J], d);
                    }
                    ++p;
                }
            }
        }
        for (unsigned r0 = 0; r0 < etot; r0 += VOL_CAP) {
            if (ec && eoff < r0 + VOL_CAP && eoff + ec > r0) {
                unsigned e = eoff - r0;                  // the place in the window; wraps below zero for elements of an earlier window
                if (full) {
                    unsigned vb[1 << N];
#pragma unroll
                    for (int m = 0; m < (1 << N); ++m) vb[m] = vbase[lin + vol_lin_off<N>(a, m)];
#pragma unroll
                    for (int sp = 0; sp < vol_nsimplex(N); ++sp, ++e) {
                        if (e >= (unsigned)VOL_CAP) continue;
                        const unsigned ch = vol_chain(N, sp);
                        const bool odd = (vol_odd(N) >> sp) & 1;
                        unsigned id[W];
#pragma unroll
                        for (int c = 0; c < W; ++c) id[c] = vb[(ch >> (3 * (odd && c >= W - 2 ? (2 * W - 3) - c : c))) & 7];
                        if (N == 3) {
                            *reinterpret_cast<uint4*>(&stage[e * W]) = make_uint4(id[0], id[1], id[2], id[W - 1]);
                        } else {
#pragma unroll
                            for (int c = 0; c < W; ++c) stage[e * W + c] = id[c];
                        }
                    }
                } else {
#pragma unroll
                    for (int sp = 0; sp < vol_nsimplex(N); ++sp) {
                        const unsigned ch = vol_chain(N, sp);
                        const bool odd = (vol_odd(N) >> sp) & 1;
                        unsigned s = 0;
#pragma unroll
                        for (int j = 0; j <= N; ++j) s |= ((in >> ((ch >> (3 * j)) & 7)) & 1) << j;
                        const unsigned long long w = N == 3 ? VOL_TET[s] : (unsigned long long)VOL_TRI[s];
                        const int cnt = (int)(w & 3);
                        for (int i = 0; i < cnt; ++i, ++e) {
                            if (e >= (unsigned)VOL_CAP) continue;
#pragma unroll
                            for (int c = 0; c < W; ++c) {
                                const int cs = odd && c >= W - 2 ? (2 * W - 3) - c : c;
                                int j, kk = -1;
                                if (N == 3) {
                                    const unsigned code = (unsigned)(w >> (2 + 4 * (4 * i + cs))) & 15;
                                    j = code;
                                    if (code >= 4) {
                                        j = (0x940u >> (2 * (code - 4))) & 3;
                                        kk = (0xFB9u >> (2 * (code - 4))) & 3;
                                    }
                                } else {
                                    const unsigned code = (unsigned)(w >> (2 + 3 * (3 * i + cs))) & 7;
                                    j = code;
                                    if (code >= 3) {
                                        j = (0x10u >> (2 * (code - 3))) & 3;
                                        kk = (0x29u >> (2 * (code - 3))) & 3;
                                    }
                                }
                                const int mj = (ch >> (3 * j)) & 7;
                                const long long J = lin + vol_lin_off<N>(a, mj);
                                unsigned id = vbase[J];
                                if (kk >= 0) id = vol_cut_id(id, emask[J], (int)((ch >> (3 * kk)) & 7) ^ mj);
                                stage[e * W + c] = id;
                            }
                        }
                    }
                }
            }
            __syncthreads();
            const unsigned nslot = (etot - r0 < (unsigned)VOL_CAP ? etot - r0 : (unsigned)VOL_CAP) * W;
            long long* dst = elems + (ebase + r0) * W;
            if (N == 3) {       // four vertex numbers per element: the run starts on 32 bytes and holds an even number of int64
                for (unsigned s = 2 * t; s < nslot; s += 512) {
                    const uint2 v = *reinterpret_cast<const uint2*>(&stage[s]);
                    *reinterpret_cast<longlong2*>(dst + s) = make_longlong2((long long)v.x, (long long)v.y);
                }
            } else {
                for (unsigned s = t; s < nslot; s += 256) dst[s] = (long long)stage[s];
            }
            __syncthreads();
        }
        ebase += etot;
        ibase += itot;
    }
}

// ---- host side
struct VolObject {
    DevBuf<double> verts;
    DevBuf<long long> elems, iface;
    long long nv = 0, ne = 0, ni = 0;
    int ndim = 0;
    hipStream_t stream = nullptr;
};

#define VOL_HIP(call, what) do { if ((call) != hipSuccess) { *err = what; delete o; return 2; } } while (0)

int vol_build(int ndim, const int n[3], long long s1, long long s2, long long origin, const double lc[3], const double h[3], double level,
              const void* phi, int f32, hipStream_t stream, VolObject** out, long long counts_out[3], const char** err) {
    if (ndim != 2 && ndim != 3) { *err = "volume_mesh: 2-D and 3-D fields only"; return 1; }
    VolArgs a;
    a.nnode = 1;
    for (int d = 0; d < 3; ++d) {
        a.n[d] = d < ndim ? n[d] : 1;
        a.lc[d] = d < ndim ? lc[d] : 0.0;
        a.h[d] = d < ndim ? h[d] : 1.0;
        if (d < ndim && n[d] < 2) { *err = "volume_mesh: at least two nodes per dimension"; return 1; }
        a.nnode *= a.n[d];
    }
    a.s1 = s1; a.s2 = ndim > 2 ? s2 : 0; a.origin = origin;
    a.level = level; a.phi = phi; a.f32 = f32;
    const long long nchunk = (a.nnode + VOL_CHUNK - 1) / VOL_CHUNK;
    if (nchunk > (1LL << 19)) { *err = "volume_mesh: the grid has too many nodes"; return 1; }     // 2^31 nodes: one vertex kernel launch

    VolObject* o = new VolObject();
    o->ndim = ndim;
    o->stream = stream;
    DevBuf<unsigned char> emask, ecnt, icnt;     // whole chunks
    DevBuf<unsigned> sums, vbase;                // [vertices | elements | interface elements] per chunk; first vertex of every node
    DevBuf<long long> off, tot;
    VOL_HIP(emask.alloc((size_t)nchunk * VOL_CHUNK), "hipMalloc(edge masks)");
    VOL_HIP(ecnt.alloc((size_t)nchunk * VOL_CHUNK), "hipMalloc(element counts)");
    VOL_HIP(icnt.alloc((size_t)nchunk * VOL_CHUNK), "hipMalloc(interface counts)");
    VOL_HIP(sums.alloc(3 * (size_t)nchunk * sizeof(unsigned)), "hipMalloc(chunk sums)");
    VOL_HIP(off.alloc(3 * (size_t)nchunk * sizeof(long long)), "hipMalloc(chunk offsets)");
    VOL_HIP(tot.alloc(3 * sizeof(long long)), "hipMalloc(totals)");
    const unsigned gchunk = (unsigned)nchunk;
    if (ndim == 2) hipLaunchKernelGGL(vol_classify_kernel<2>, dim3(gchunk), dim3(256), 0, stream, a, emask.p, ecnt.p, icnt.p, sums.p, nchunk);
    else hipLaunchKernelGGL(vol_classify_kernel<3>, dim3(gchunk), dim3(256), 0, stream, a, emask.p, ecnt.p, icnt.p, sums.p, nchunk);
    hipLaunchKernelGGL(vol_scan_kernel, dim3(1), dim3(1024), 0, stream, sums.p, nchunk, off.p, tot.p);
    long long th[3] = {0, 0, 0};
    VOL_HIP(hipMemcpyAsync(th, tot, 3 * sizeof(long long), hipMemcpyDeviceToHost, stream), "volume_mesh: counts");
    VOL_HIP(hipStreamSynchronize(stream), "volume_mesh: counts");
    o->nv = th[0];
    o->ne = th[1];
    o->ni = th[2];
    if (o->nv > 0xffffffffLL) { *err = "volume_mesh: more than 2^32 vertices"; delete o; return 1; }
    if (o->nv) {
        VOL_HIP(vbase.alloc((size_t)nchunk * VOL_CHUNK * sizeof(unsigned)), "hipMalloc(vertex offsets)");
        VOL_HIP(o->verts.alloc((size_t)o->nv * ndim * sizeof(double)), "hipMalloc(vertices)");
        VOL_HIP(o->elems.alloc((size_t)std::max(o->ne, 1LL) * (ndim + 1) * sizeof(long long)), "hipMalloc(elements)");
        VOL_HIP(o->iface.alloc((size_t)std::max(o->ni, 1LL) * ndim * sizeof(long long)), "hipMalloc(interface elements)");
        hipLaunchKernelGGL(vol_offset_kernel, dim3(gchunk), dim3(256), 0, stream, emask.p, off.p, vbase.p);
        const unsigned gnode = (unsigned)((a.nnode + 255) / 256);
        if (ndim == 2) {
            hipLaunchKernelGGL(vol_vertex_kernel<2>, dim3(gnode), dim3(256), 0, stream, a, emask.p, vbase.p, o->verts.p);
            hipLaunchKernelGGL(vol_element_kernel<2>, dim3(gchunk), dim3(256), 0, stream, a, emask.p, ecnt.p, icnt.p, vbase.p, off.p, nchunk,
                               o->elems.p, o->iface.p);
        } else {
            hipLaunchKernelGGL(vol_vertex_kernel<3>, dim3(gnode), dim3(256), 0, stream, a, emask.p, vbase.p, o->verts.p);
            hipLaunchKernelGGL(vol_element_kernel<3>, dim3(gchunk), dim3(256), 0, stream, a, emask.p, ecnt.p, icnt.p, vbase.p, off.p, nchunk,
                               o->elems.p, o->iface.p);
        }
    }
    VOL_HIP(hipGetLastError(), "volume_mesh: launch failed");
    VOL_HIP(hipStreamSynchronize(stream), "volume_mesh: device error");     // the work buffers are released on return
    counts_out[0] = o->nv;
    counts_out[1] = o->ne;
    counts_out[2] = o->ni;
    *out = o;
    return 0;
}
#undef VOL_HIP

int vol_read(VolObject* o, double* verts, long long* elems, long long* iface, const char** err) {
    hipError_t e = hipSuccess;
    if (verts && o->nv) e = hipMemcpyAsync(verts, o->verts, (size_t)o->nv * o->ndim * sizeof(double), hipMemcpyDeviceToDevice, o->stream);
    if (elems && o->ne && e == hipSuccess)
        e = hipMemcpyAsync(elems, o->elems, (size_t)o->ne * (o->ndim + 1) * sizeof(long long), hipMemcpyDeviceToDevice, o->stream);
    if (iface && o->ni && e == hipSuccess)
        e = hipMemcpyAsync(iface, o->iface, (size_t)o->ni * o->ndim * sizeof(long long), hipMemcpyDeviceToDevice, o->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) { *err = "volume_mesh read: device error"; return 2; }
    return 0;
}

void vol_free(VolObject* o) { delete o; }

}  // namespace lsm
