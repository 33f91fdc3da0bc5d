// lsm_iso.hip — isosurface(ϕ, level) on the device: the interface {ϕ = level} as an indexed mesh (segments in 2-D, triangles
// in 3-D), what ext/MMGSurfaceExt.jl:48-50 gets from marching cubes and ext/MakieExt.jl from contour!.  Marching simplices on
// the Freudenthal (Kuhn) subdivision of every cell: a watertight and consistently oriented mesh of the zero set of the
// piecewise-linear interpolant, shared vertices.  The subdivision, the sign convention, the cut vertices and
// the element tables are kuhn.h's; tests/_iso_ref.py restates them and what this file adds:
//   * an edge carries a vertex only if an active cell contains it (dense: every cell; band: the cells whose 2^N corners are
//     band nodes — only band values decide); vertices are numbered by ascending node (axis 0 fastest), then ascending d;
//   * the elements are those of the active cells, ascending.
// Kernels: kuhn.h's classify sweep with the band's cover test (sums per chunk: vertices, elements, nodes that own any), scan.h's
// scan of the chunk sums, an ordered compaction of the nodes that own a vertex or an element (with their vertex and element offsets;
// the vertex offset also goes into a node-indexed array that is written and read at those nodes only), and one thread per
// listed node for the vertices and for the elements.  No atomic decides an output position.  The host side of kuhn.h (the front
// half of a build, the read-out) is defined here.
#include <algorithm>
#include <memory>

#include "kuhn.h"
#include "scan.h"

namespace lsm {

// is the cell anchored at I − m' in the grid with all its corners on the band?
template <int N>
__device__ __forceinline__ bool iso_cell_active(const KuhnArgs& a, const int I[3], int mp) {
    const int C[3] = {I[0] - (mp & 1), I[1] - ((mp >> 1) & 1), N > 2 ? I[2] - ((mp >> 2) & 1) : 0};
#pragma unroll
    for (int d = 0; d < N; ++d)
        if (C[d] < 0 || C[d] + 1 >= a.n[d]) return false;
    const long long q = kuhn_node<N>(a, C);
    bool act = true;
    for (int m = 0; m < (1 << N); ++m) act = act && a.mask[q + kuhn_off<N>(a, m)] != 0;
    return act;
}
// elements of the cell whose corners have the inside flags `in` (bit m = corner m)
template <int N>
__device__ __forceinline__ unsigned iso_count(unsigned in) {
    unsigned c = 0;
#pragma unroll
    for (int p = 0; p < kuhn_nsimplex(N); ++p) {
        const unsigned ch = kuhn_chain(N, p);
        unsigned k = 0;
#pragma unroll
        for (int j = 0; j <= N; ++j) k += (in >> ((ch >> (3 * j)) & 7)) & 1;
        c += (k == 0 || k == N + 1) ? 0u : (N == 3 && k == 2 ? 2u : 1u);
    }
    return c;
}

// per node: the edges it owns that carry a vertex (bit d − 1) and the elements of the cell it anchors; per chunk the numbers of
// vertices, elements and nodes that own any
template <int N>
__global__ void __launch_bounds__(256) iso_classify_kernel(KuhnArgs a, unsigned char* emask, unsigned char* ecnt, unsigned* sums, long long nchunk) {
    const long long c0 = (long long)blockIdx.x * KUHN_CHUNK;
    unsigned nv = 0, ne = 0, nl = 0;
    int I[3];
    kuhn_unlin<N>(a, c0 + threadIdx.x < a.nnode ? c0 + threadIdx.x : a.nnode - 1, I);
    for (int k = 0; k < KUHN_PER; ++k) {
        const long long lin = c0 + threadIdx.x + 256 * k;
        const bool valid = lin < a.nnode;
        const unsigned up = valid ? kuhn_up<N>(a, I) : 0u;
        const unsigned in = kuhn_inside<N>(a, kuhn_node<N>(a, I), up, valid);
        unsigned em = 0, ec = 0;
        if (valid) {
            em = kuhn_edges<N>(in, up);
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
        kuhn_advance<N>(a, I);
    }
    kuhn_chunk_sums(nv, ne, nl, sums, nchunk);
}

// the nodes of every chunk that own a vertex or an element, ascending, at the chunk's scanned offset: node, vertex offset,
// element offset; vbase[node] := vertex offset where the node owns a vertex
__global__ void __launch_bounds__(256) iso_compact_kernel(const unsigned char* emask, const unsigned char* ecnt, long long nnode, const long long* off,
                                                          long long nchunk, long long* list, long long* list_v, long long* list_e, unsigned* vbase) {
    __shared__ unsigned wsum[3][4];
    const int t = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * KUHN_CHUNK + (long long)t * KUHN_PER;
    const uint4 em4 = *reinterpret_cast<const uint4*>(emask + c0), ec4 = *reinterpret_cast<const uint4*>(ecnt + c0);
    const unsigned emw[4] = {em4.x, em4.y, em4.z, em4.w}, ecw[4] = {ec4.x, ec4.y, ec4.z, ec4.w};
    unsigned m[3] = {0, 0, 0};
#pragma unroll
    for (int e = 0; e < KUHN_PER; ++e) {
        const unsigned em = (emw[e / 4] >> (8 * (e % 4))) & 255u, ec = (ecw[e / 4] >> (8 * (e % 4))) & 255u;
        m[0] += __popc(em);
        m[1] += ec;
        m[2] += (em | ec) != 0;
    }
    unsigned total;
    long long pv = off[blockIdx.x] + block_excl_scan<4>(m[0], wsum[0], total), pe = off[nchunk + blockIdx.x] + block_excl_scan<4>(m[1], wsum[1], total),
              pl = off[2 * nchunk + blockIdx.x] + block_excl_scan<4>(m[2], wsum[2], total);
#pragma unroll
    for (int e = 0; e < KUHN_PER; ++e) {
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
__global__ void __launch_bounds__(256) iso_vertex_kernel(KuhnArgs a, const unsigned char* emask, const long long* list, const long long* list_v,
                                                         long long nlist, double* verts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nlist) return;
    const long long lin = list[i];
    const unsigned em = emask[lin];
    if (!em) return;
    int I[3];
    kuhn_unlin<N>(a, lin, I);
    double x[3];
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = a.lc[e] + (double)I[e] * a.h[e];
    kuhn_cut_vertices<N>(a, kuhn_node<N>(a, I), x, em, list_v[i], verts);
}

// the elements of the cell a listed node anchors
template <int N>
__global__ void __launch_bounds__(256) iso_element_kernel(KuhnArgs a, const unsigned char* emask, const unsigned char* ecnt, const unsigned* vbase,
                                                          const long long* list, const long long* list_e, long long nlist, long long* elems) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nlist) return;
    const long long lin = list[i];
    if (!ecnt[lin]) return;
    int I[3];
    kuhn_unlin<N>(a, lin, I);
    const long long q = kuhn_node<N>(a, I);
    unsigned in = 0;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) in |= ld_val(a.phi, q + kuhn_off<N>(a, m), a.f32) < a.level ? 1u << m : 0u;
    kuhn_interface_elements<N>(a, elems, lin, in, list_e[i],
                               [&](long long J, int d) { return (long long)vbase[J] + __popc(emask[J] & ((1u << (d - 1)) - 1u)); });
}

// ---- host side: kuhn.h's
int kuhn_begin(const LsmHandle* h, double level, const void* phi, const unsigned char* mask, long long max_chunks, const char* const msg[5],
               KuhnWork& w, const char** err) {
    const int ndim = h->grid.ndim;
    if (ndim != 2 && ndim != 3) { *err = msg[0]; return 1; }
    KuhnArgs& a = w.a;
    a.nnode = 1;
    for (int d = 0; d < 3; ++d) {
        a.n[d] = d < ndim ? h->nloc[d] : 1;
        a.lc[d] = d < ndim ? h->grid.lc[d] : 0.0;
        a.h[d] = d < ndim ? h->h[d] : 1.0;
        if (d < ndim && a.n[d] < 2) { *err = msg[1]; return 1; }
        a.nnode *= a.n[d];
    }
    a.s1 = h->lay.stride[1]; a.s2 = ndim > 2 ? h->lay.stride[2] : 0; a.origin = h->lay.origin;
    a.level = level; a.phi = phi; a.f32 = h->dtype == LSM_DTYPE_F32; a.mask = mask;
    w.nchunk = (a.nnode + KUHN_CHUNK - 1) / KUHN_CHUNK;
    if (w.nchunk > max_chunks) { *err = msg[2]; return 1; }
    MOD_HIP(w.emask.alloc((size_t)w.nchunk * KUHN_CHUNK), "hipMalloc(edge masks)");
    MOD_HIP(w.ecnt.alloc((size_t)w.nchunk * KUHN_CHUNK), "hipMalloc(element counts)");
    MOD_HIP(w.sums.alloc(3 * (size_t)w.nchunk * sizeof(unsigned)), "hipMalloc(chunk sums)");
    MOD_HIP(w.off.alloc(3 * (size_t)w.nchunk * sizeof(long long)), "hipMalloc(chunk offsets)");
    MOD_HIP(w.tot.alloc(3 * sizeof(long long)), "hipMalloc(totals)");
    return 0;
}

int kuhn_totals(KuhnWork& w, hipStream_t stream, const char* const msg[5], const char** err) {
    const long long n = w.nchunk;
    chunk_scan<3, long long>(stream, {{{w.sums.p, w.off.p, 0}, {w.sums.p + n, w.off.p + n, 0}, {w.sums.p + 2 * n, w.off.p + 2 * n, 0}}}, n, w.tot.p);
    MOD_HIP(hipMemcpyAsync(w.total, w.tot, 3 * sizeof(long long), hipMemcpyDeviceToHost, stream), msg[3]);
    MOD_HIP(hipStreamSynchronize(stream), msg[3]);
    if (w.total[0] > 0xffffffffLL) { *err = msg[4]; return 1; }
    return 0;
}

int kuhn_read(hipStream_t stream, std::initializer_list<KuhnCopy> copies, const char* what, const char** err) {
    for (const KuhnCopy& c : copies)
        if (c.dst && c.bytes) MOD_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, stream), what);
    MOD_HIP(hipStreamSynchronize(stream), what);
    return 0;
}

// ---- host side: isosurface's
struct IsoObject {
    DevBuf<double> verts;
    DevBuf<long long> elems;
    long long nv = 0, ne = 0;
    int ndim = 0;
    hipStream_t stream = nullptr;
};

int iso_build(const LsmHandle* h, double level, const void* phi, const unsigned char* mask, IsoObject** out, long long counts_out[2], const char** err) {
    static const char* const msg[5] = {"isosurface: 2-D and 3-D fields only", "isosurface: at least two nodes per dimension",
                                       "isosurface: the grid has too many nodes", "isosurface: counts", "isosurface: more than 2^32 vertices"};
    const hipStream_t stream = h->stream;
    const int ndim = h->grid.ndim;
    KuhnWork w;
    if (const int r = kuhn_begin(h, level, phi, mask, 1LL << 23, msg, w, err)) return r;     // 256 threads per chunk in one launch
    LSM_LAUNCH_ND(ndim, iso_classify_kernel, (unsigned)w.nchunk, 256, stream, w.a, w.emask.p, w.ecnt.p, w.sums.p, w.nchunk);
    if (const int r = kuhn_totals(w, stream, msg, err)) return r;
    const KuhnArgs& a = w.a;
    std::unique_ptr<IsoObject> o(new IsoObject());
    o->ndim = ndim;
    o->stream = stream;
    o->nv = w.total[0];
    o->ne = w.total[1];
    const long long nlist = w.total[2];
    if (nlist) {
        DevBuf<unsigned> vbase;          // vertex offset of a node that owns a vertex
        DevBuf<long long> list, list_v, list_e;
        MOD_HIP(vbase.alloc((size_t)a.nnode * sizeof(unsigned)), "hipMalloc(vertex offsets)");
        MOD_HIP(list.alloc((size_t)nlist * sizeof(long long)), "hipMalloc(node list)");
        MOD_HIP(list_v.alloc((size_t)nlist * sizeof(long long)), "hipMalloc(node list)");
        MOD_HIP(list_e.alloc((size_t)nlist * sizeof(long long)), "hipMalloc(node list)");
        MOD_HIP(o->verts.alloc((size_t)std::max(o->nv, 1LL) * ndim * sizeof(double)), "hipMalloc(vertices)");
        MOD_HIP(o->elems.alloc((size_t)std::max(o->ne, 1LL) * ndim * sizeof(long long)), "hipMalloc(elements)");
        hipLaunchKernelGGL(iso_compact_kernel, dim3((unsigned)w.nchunk), dim3(256), 0, stream, w.emask.p, w.ecnt.p, a.nnode, w.off.p, w.nchunk, list.p,
                           list_v.p, list_e.p, vbase.p);
        const unsigned glist = (unsigned)((nlist + 255) / 256);
        LSM_LAUNCH_ND(ndim, iso_vertex_kernel, glist, 256, stream, a, w.emask.p, list.p, list_v.p, nlist, o->verts.p);
        LSM_LAUNCH_ND(ndim, iso_element_kernel, glist, 256, stream, a, w.emask.p, w.ecnt.p, vbase.p, list.p, list_e.p, nlist, o->elems.p);
    }
    MOD_HIP(hipGetLastError(), "isosurface: launch failed");
    MOD_HIP(hipStreamSynchronize(stream), "isosurface: device error");     // the work buffers are released on return
    counts_out[0] = o->nv;
    counts_out[1] = o->ne;
    *out = o.release();
    return 0;
}

int iso_read(IsoObject* o, double* verts, long long* elems, const char** err) {
    return kuhn_read(o->stream, {{verts, o->verts, (size_t)o->nv * o->ndim * sizeof(double)}, {elems, o->elems, (size_t)o->ne * o->ndim * sizeof(long long)}},
                     "isosurface read: device error", err);
}

void iso_free(IsoObject* o) { delete o; }

}  // namespace lsm
