// lsm_vol.hip — volume_mesh(ϕ, level) on the device: the body-fitted simplicial mesh of the interior {ϕ < level} (triangles in
// 2-D, tetrahedra in 3-D) whose boundary inside the box is isosurface's mesh — the splitting phase of mmg2d_O3 / mmg3d_O3 -ls that
// ext/MMGVolumeExt.jl (export_volume_mesh) runs over the Kuhn triangulation of the grid, without the remesher.
// The subdivision, the sign convention, the cut vertices and the interface elements are kuhn.h's, shared with lsm_iso.hip;
// tests/_vol_ref.py restates what this file adds:
//   * node I (ascending, axis 0 fastest) owns itself if ϕ[I] < level, at lc + i·h, then the cut vertices of its edges;
//   * cells ascending, simplices in permutation order; with a < b < … the inside and c < d the outside corners by chain position
//     a simplex gives itself (all inside), nothing (none), (a, ac, ad) or (a, b, bc), (a, bc, ac) in 2-D, (a, ab', ac', ad'), the
//     prism u = (a, ac, ad), w = (b, bc, bd) or the prism u = (a, b, c), w = (ad, bd, cd) in 3-D, a prism being cut as
//     (u0, u1, u2, w2), (u0, u1, w1, w2), (u0, w0, w1, w2): no Steiner point, neighbours pick the same diagonals, the interface
//     quad is cut as isosurface cuts it;
//   * the last two vertices of an element are swapped by a table over (sign pattern, sub-element) xor the parity of π (never a
//     geometric test): every signed volume is >= 0;
//   * the interface elements are isosurface's, in its order and orientation, in this mesh's vertex numbering.
// Kernels: kuhn.h's classify sweep (the edge mask with the inside bit, a byte of interface count next to the element count; sums
// per chunk: vertices, elements, interface elements), the scan of the chunk sums, the vertex offset of every node (a scan
// inside the chunk on top of the chunk's base), one thread per node for the vertices, and one workgroup per chunk for the
// elements: it scans the counts of 256 cells at a time, stages their elements in LDS as 32-bit vertex numbers and writes the
// stage out as one contiguous run of int64, 16 bytes per lane.  No atomic decides an output position.
#include <algorithm>
#include <memory>

#include "kuhn.h"

namespace lsm {

constexpr int VOL_CAP = 2048;              // elements the LDS stage holds: 256 interior cells of 6 tetrahedra fit in one round

// sub-elements per sign pattern (bit j = chain corner j inside) on an even permutation, the orientation table applied: bits 0..1 the
// count, then N + 1 vertex codes per sub-element; an odd permutation swaps the last two vertices.  3-D codes, 4 bits: 0..3 the
// chain corner, 4 + the edge (j, k) in the order 01, 02, 03, 12, 13, 23.  2-D codes, 3 bits: 0..2 the corner, 3 + the edge in the
// order 01, 02, 12.
__device__ const unsigned long long VOL_TET[16] = {
    0x0ull, 0x19501ull, 0x1e105ull, 0x21c41e1421943ull, 0x25d49ull, 0x1e4825d01a503ull, 0x2548565066107ull, 0x2618224424843ull,
    0x2258dull, 0x260c225025503ull, 0x1a4c65905e507ull, 0x1e5425c40e443ull, 0x218c9a14a1d4bull, 0x21d01e0820c83ull, 0x159059484d887ull,
    0xc841ull};
__device__ const unsigned VOL_TRI[8] = {0x0u, 0x461u, 0x3a5u, 0x94522u, 0x589u, 0xac2a2u, 0x70c46u, 0x221u};

// elements and interface elements of the cell whose corners have the inside flags `in` (bit m = corner m): bits 0..7 and 8..15
template <int N>
__device__ __forceinline__ unsigned vol_count(unsigned in) {
    unsigned c = 0;
#pragma unroll
    for (int p = 0; p < kuhn_nsimplex(N); ++p) {
        const unsigned ch = kuhn_chain(N, p);
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
// elements of the cell it anchors; per chunk the numbers of vertices, elements and interface elements
template <int N>
__global__ void __launch_bounds__(256) vol_classify_kernel(KuhnArgs a, unsigned char* emask, unsigned char* ecnt, unsigned char* icnt, unsigned* sums,
                                                           long long nchunk) {
    const long long c0 = (long long)blockIdx.x * KUHN_CHUNK;
    unsigned nv = 0, ne = 0, ni = 0;
    int I[3];
    kuhn_unlin<N>(a, c0 + threadIdx.x < a.nnode ? c0 + threadIdx.x : a.nnode - 1, I);
    for (int k = 0; k < KUHN_PER; ++k) {
        const long long lin = c0 + threadIdx.x + 256 * k;
        const bool valid = lin < a.nnode;
        const unsigned up = valid ? kuhn_up<N>(a, I) : 0u;
        const unsigned in = kuhn_inside<N>(a, kuhn_node<N>(a, I), up, valid);
        unsigned em = 0, ec = 0, ic = 0;
        if (valid) {
            em = kuhn_edges<N>(in, up);
            if (up == (1u << N) - 1) {
                if (em) {
                    const unsigned c = vol_count<N>(in);
                    ec = c & 255u;
                    ic = c >> 8;
                } else if (in & 1) {
                    ec = kuhn_nsimplex(N);       // every corner inside
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
        kuhn_advance<N>(a, I);
    }
    kuhn_chunk_sums(nv, ne, ni, sums, nchunk);
}

// vbase[node] := the number of the first vertex the node owns: the chunk's scanned base plus a scan inside the chunk.  A thread
// takes KUHN_PER consecutive nodes; the arrays cover whole chunks.
__global__ void __launch_bounds__(256) vol_offset_kernel(const unsigned char* emask, const long long* off, unsigned* vbase) {
    __shared__ unsigned wsum[4];
    const int t = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * KUHN_CHUNK + (long long)t * KUHN_PER;
    const uint4 em4 = *reinterpret_cast<const uint4*>(emask + c0);
    const unsigned emw[4] = {em4.x, em4.y, em4.z, em4.w};
    unsigned m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) m += __popc(emw[w]);
    unsigned total;
    unsigned p = (unsigned)off[blockIdx.x] + block_excl_scan<4>(m, wsum, total);
    unsigned o[KUHN_PER];
#pragma unroll
    for (int e = 0; e < KUHN_PER; ++e) {
        o[e] = p;
        p += __popc((emw[e / 4] >> (8 * (e % 4))) & 255u);
    }
#pragma unroll
    for (int e = 0; e < KUHN_PER; e += 4) *reinterpret_cast<uint4*>(vbase + c0 + e) = make_uint4(o[e], o[e + 1], o[e + 2], o[e + 3]);
}

// the vertices a node owns: itself if inside, then the cut vertices of its edges
template <int N>
__global__ void __launch_bounds__(256) vol_vertex_kernel(KuhnArgs a, const unsigned char* emask, const unsigned* vbase, double* verts) {
    const long long lin = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lin >= a.nnode) return;
    const unsigned em = emask[lin];
    if (!em) return;
    int I[3];
    kuhn_unlin<N>(a, lin, I);
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
    kuhn_cut_vertices<N>(a, kuhn_node<N>(a, I), x, em, p, verts);
}

// the elements and the interface elements of a chunk's cells.  256 cells per pass: their counts are scanned in the workgroup, every
// thread puts the elements of its cell into the LDS stage at their place (32-bit vertex numbers), and the workgroup writes the
// stage to the pass's contiguous run of the output, consecutive lanes to consecutive addresses.  A pass with more than VOL_CAP
// elements (cut cells give up to 18) takes several rounds over windows of VOL_CAP elements.  The interface elements, a surface's
// worth, are written by their threads directly.
template <int N>
__global__ void __launch_bounds__(256) vol_element_kernel(KuhnArgs a, const unsigned char* emask, const unsigned char* ecnt, const unsigned char* icnt,
                                                          const unsigned* vbase, const long long* off, long long nchunk, long long* elems,
                                                          long long* iface) {
    constexpr int W = N + 1;
    __shared__ __attribute__((aligned(16))) unsigned stage[VOL_CAP * W];
    __shared__ unsigned wsum[2][4];
    const int t = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * KUHN_CHUNK;
    long long ebase = off[nchunk + blockIdx.x], ibase = off[2 * nchunk + blockIdx.x];
    for (int k = 0; k < KUHN_PER; ++k) {
        const long long lin = c0 + t + 256 * k;          // the count arrays cover whole chunks, zero past the last node
        const unsigned ec = ecnt[lin], ic = icnt[lin];
        const unsigned x = ec | (ic << 16);              // at most 256·18 and 256·12 per pass: two 16-bit sums in one word
        unsigned total;
        const unsigned excl = block_excl_scan<4>(x, wsum[k & 1], total);    // two buffers: a pass has no barrier after the scan
        const unsigned eoff = excl & 0xffffu, ioff = excl >> 16, etot = total & 0xffffu, itot = total >> 16;
        if (!etot) continue;                             // uniform; no elements, no interface
        const bool full = ec == (unsigned)kuhn_nsimplex(N) && ic == 0;      // no simplex is cut and all are kept: every corner inside
        unsigned in = 0;
        if (ec && !full) {
#pragma unroll
            for (int m = 0; m < (1 << N); ++m) in |= (unsigned)(emask[lin + kuhn_lin_off<N>(a, m)] >> 7) << m;
        }
        if (ic)
            kuhn_interface_elements<N>(a, iface, lin, in, ibase + ioff,
                                       [&](long long J, int d) { return (long long)vol_cut_id(vbase[J], emask[J], d); });
        for (unsigned r0 = 0; r0 < etot; r0 += VOL_CAP) {
            if (ec && eoff < r0 + VOL_CAP && eoff + ec > r0) {
                unsigned e = eoff - r0;                  // the place in the window; wraps below zero for elements of an earlier window
                if (full) {
                    unsigned vb[1 << N];
#pragma unroll
                    for (int m = 0; m < (1 << N); ++m) vb[m] = vbase[lin + kuhn_lin_off<N>(a, m)];
#pragma unroll
                    for (int sp = 0; sp < kuhn_nsimplex(N); ++sp, ++e) {
                        if (e >= (unsigned)VOL_CAP) continue;
                        const unsigned ch = kuhn_chain(N, sp);
                        const bool odd = (kuhn_odd(N) >> sp) & 1;
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
                    for (int sp = 0; sp < kuhn_nsimplex(N); ++sp) {
                        const unsigned ch = kuhn_chain(N, sp);
                        const bool odd = (kuhn_odd(N) >> sp) & 1;
                        const unsigned long long w = N == 3 ? VOL_TET[kuhn_pattern<N>(in, ch)] : (unsigned long long)VOL_TRI[kuhn_pattern<N>(in, ch)];
                        const int cnt = (int)(w & 3);
                        for (int i = 0; i < cnt; ++i, ++e) {
                            if (e >= (unsigned)VOL_CAP) continue;
#pragma unroll
                            for (int c = 0; c < W; ++c) {
                                const int cs = odd && c >= W - 2 ? (2 * W - 3) - c : c;
                                // a vertex code: a chain corner, or past the corners an edge code
                                const unsigned code = N == 3 ? (unsigned)(w >> (2 + 4 * (4 * i + cs))) & 15 : (unsigned)(w >> (2 + 3 * (3 * i + cs))) & 7;
                                int j = code, kk = -1;
                                if (code > (unsigned)N) kuhn_edge<N>(code - (N + 1), j, kk);
                                const int mj = (ch >> (3 * j)) & 7;
                                const long long J = lin + kuhn_lin_off<N>(a, mj);
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

int vol_build(const LsmHandle* h, double level, const void* phi, VolObject** out, long long counts_out[3], const char** err) {
    static const char* const msg[5] = {"volume_mesh: 2-D and 3-D fields only", "volume_mesh: at least two nodes per dimension",
                                       "volume_mesh: the grid has too many nodes", "volume_mesh: counts", "volume_mesh: more than 2^32 vertices"};
    const hipStream_t stream = h->stream;
    const int ndim = h->grid.ndim;
    KuhnWork w;
    DevBuf<unsigned char> icnt;     // whole chunks
    if (const int r = kuhn_begin(h, level, phi, nullptr, 1LL << 19, msg, w, err)) return r;     // 2^31 nodes: one vertex kernel launch
    MOD_HIP(icnt.alloc((size_t)w.nchunk * KUHN_CHUNK), "hipMalloc(interface counts)");
    LSM_LAUNCH_ND(ndim, vol_classify_kernel, (unsigned)w.nchunk, 256, stream, w.a, w.emask.p, w.ecnt.p, icnt.p, w.sums.p, w.nchunk);
    if (const int r = kuhn_totals(w, stream, msg, err)) return r;
    const KuhnArgs& a = w.a;
    std::unique_ptr<VolObject> o(new VolObject());
    o->ndim = ndim;
    o->stream = stream;
    o->nv = w.total[0];
    o->ne = w.total[1];
    o->ni = w.total[2];
    if (o->nv) {
        const unsigned gchunk = (unsigned)w.nchunk;
        DevBuf<unsigned> vbase;     // first vertex of every node
        MOD_HIP(vbase.alloc((size_t)w.nchunk * KUHN_CHUNK * sizeof(unsigned)), "hipMalloc(vertex offsets)");
        MOD_HIP(o->verts.alloc((size_t)o->nv * ndim * sizeof(double)), "hipMalloc(vertices)");
        MOD_HIP(o->elems.alloc((size_t)std::max(o->ne, 1LL) * (ndim + 1) * sizeof(long long)), "hipMalloc(elements)");
        MOD_HIP(o->iface.alloc((size_t)std::max(o->ni, 1LL) * ndim * sizeof(long long)), "hipMalloc(interface elements)");
        hipLaunchKernelGGL(vol_offset_kernel, dim3(gchunk), dim3(256), 0, stream, w.emask.p, w.off.p, vbase.p);
        const unsigned gnode = (unsigned)((a.nnode + 255) / 256);
        LSM_LAUNCH_ND(ndim, vol_vertex_kernel, gnode, 256, stream, a, w.emask.p, vbase.p, o->verts.p);
        LSM_LAUNCH_ND(ndim, vol_element_kernel, gchunk, 256, stream, a, w.emask.p, w.ecnt.p, icnt.p, vbase.p, w.off.p, w.nchunk, o->elems.p, o->iface.p);
    }
    MOD_HIP(hipGetLastError(), "volume_mesh: launch failed");
    MOD_HIP(hipStreamSynchronize(stream), "volume_mesh: device error");     // the work buffers are released on return
    counts_out[0] = o->nv;
    counts_out[1] = o->ne;
    counts_out[2] = o->ni;
    *out = o.release();
    return 0;
}

int vol_read(VolObject* o, double* verts, long long* elems, long long* iface, const char** err) {
    return kuhn_read(o->stream, {{verts, o->verts, (size_t)o->nv * o->ndim * sizeof(double)},
                                 {elems, o->elems, (size_t)o->ne * (o->ndim + 1) * sizeof(long long)},
                                 {iface, o->iface, (size_t)o->ni * o->ndim * sizeof(long long)}}, "volume_mesh read: device error", err);
}

void vol_free(VolObject* o) { delete o; }

}  // namespace lsm
