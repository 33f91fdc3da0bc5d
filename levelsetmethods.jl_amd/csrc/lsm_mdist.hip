// lsm_mdist.hip — mesh_distance(mesh, grid, cutoff) on the device: ϕ[I] = s(I)·min(d(I), c), the signed distance from every grid
// node to a closed, consistently oriented mesh (segments in 2-D, triangles in 3-D, oriented as isosurface orients them: normals
// from inside to outside) — the inverse of lsm_iso.hip.  DESIGN.md §7.14; tests/_mdist_ref.py restates every operation, in this
// file's operation order (built with -ffp-contract=off: the device rounds as numpy does).  The rules:
//   * node I sits at lc + I·h; d² is the squared distance to the closest point of the nearest element: Ericson's region
//     classification (vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, interior) in 3-D, the clamped projection in 2-D;
//     a NaN (an element of zero size that reaches a division) never wins the minimum;
//   * the sign is a crossing count along axis 0 and does not depend on the closest feature: a grid line (j[, k]) hits an element
//     iff its (y[, z]) lies in the element's projection, counted half-open so that a line through a shared edge or vertex is
//     counted once (2-D: (a_y > y) != (b_y > y); 3-D: edge functions evaluated from the lower vertex number, top-left rule on
//     zeros); a hit at ξ adds −σ (σ: sign of the outward normal along axis 0) to the flip counter of the first node with
//     x_i >= ξ, slot 0 left of the grid, slot n0 right of it; the winding count of a node is the prefix sum of its line's slots;
//   * s = −1 where the winding count is non-zero; a line whose n0 + 1 slots do not sum to zero is counted as unbalanced.
// Kernels: md_prep (reads only: element numbers in range, vertices finite, the largest number of pieces an element's box needs),
// md_init, md_dist (one wave per (element, piece of its box dilated by c): atomicMin on the bit pattern of d²), md_sign (8 lanes
// per element over the lines of its projection: integer atomicAdd), md_final (one wave per grid row: prefix sum, sqrt, store).
// Minima and integer sums do not depend on the order of arrival: the result is deterministic bit for bit.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lsm_handle.h"
#include "wave.h"

namespace lsm {

constexpr int MD_PIECE = 2048;            // nodes per work item of the distance pass: 32 per lane
constexpr int MD_SUB = 8;                 // lanes per element in the sign pass
constexpr double MD_MARGIN = 1.0 / 1024;  // index ranges are widened by this fraction of a node: a superset in spite of rounding
constexpr long long MD_MAX_BLOCKS = 1LL << 24;
enum { MD_BAD_INDEX = 0, MD_NONFINITE = 1, MD_MAXPIECES = 2, MD_NEAR = 3, MD_UNBALANCED = 4, MD_SKIPPED = 5, MD_NSTAT = 8 };

struct MdArgs {
    int n[3];
    long long s1, s2, origin;   // the padded layout of ϕ
    long long nnode, nrow;
    double lc[3], h[3];
    double c;
    unsigned long long c2bits;  // the bit pattern of c·c
    long long nv, ne;
    const double* verts;
    const long long* elems;
};

// the nodes lo..hi of one axis within [mn, mx] (a superset by MD_MARGIN of a node); hi < lo: none
__device__ __forceinline__ void md_range(double mn, double mx, double lc, double h, int n, int& lo, int& hi) {
    const double tlo = (mn - lc) / h - MD_MARGIN, thi = (mx - lc) / h + MD_MARGIN, last = (double)(n - 1);
    lo = !(tlo > 0.0) ? 0 : (tlo > last ? n : (int)ceil(tlo));
    hi = !(thi < last) ? n - 1 : (thi < 0.0 ? -1 : (int)floor(thi));
}

// the element's vertex numbers; false if one is out of range
template <int N>
__device__ __forceinline__ bool md_indices(const MdArgs& a, long long e, long long g[N]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        g[k] = a.elems[e * N + k];
        ok = ok && g[k] >= 0 && g[k] < a.nv;
    }
    return ok;
}
template <int N>
__device__ __forceinline__ void md_vertices(const MdArgs& a, const long long g[N], double v[N][N]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int d = 0; d < N; ++d) v[k][d] = a.verts[g[k] * N + d];
}
// the nodes within c of the element's bounding box; returns their number
template <int N>
__device__ __forceinline__ long long md_box(const MdArgs& a, const double v[N][N], int lo[3], int hi[3]) {
    long long vol = 1;
    lo[2] = hi[2] = 0;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        double mn = v[0][d], mx = v[0][d];
#pragma unroll
        for (int k = 1; k < N; ++k) { mn = fmin(mn, v[k][d]); mx = fmax(mx, v[k][d]); }
        md_range(mn - a.c, mx + a.c, a.lc[d], a.h[d], a.n[d], lo[d], hi[d]);
        vol *= hi[d] >= lo[d] ? (long long)(hi[d] - lo[d] + 1) : 0LL;
    }
    return vol;
}

// reads only.  Thread i: vertex i is finite; element i has its numbers in range; the pieces its box needs.
template <int N>
__global__ void __launch_bounds__(256) md_prep_kernel(MdArgs a, unsigned long long* st) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < a.nv) {
        bool fin = true;
#pragma unroll
        for (int d = 0; d < N; ++d) fin = fin && isfinite(a.verts[i * N + d]);
        if (!fin) atomicAdd(&st[MD_NONFINITE], 1ULL);
    }
    if (i >= a.ne) return;
    long long g[N];
    if (!md_indices<N>(a, i, g)) { atomicAdd(&st[MD_BAD_INDEX], 1ULL); return; }
    double v[N][N];
    md_vertices<N>(a, g, v);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int d = 0; d < N; ++d) fin = fin && isfinite(v[k][d]);
    if (!fin) return;           // reported through its vertex
    int lo[3], hi[3];
    const unsigned long long pieces = (unsigned long long)((md_box<N>(a, v, lo, hi) + MD_PIECE - 1) / MD_PIECE);
    if (pieces > st[MD_MAXPIECES]) atomicMax(&st[MD_MAXPIECES], pieces);
}

__global__ void __launch_bounds__(256) md_init_kernel(unsigned long long* d2, long long nnode, unsigned long long c2bits) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nnode) d2[i] = c2bits;
}

__device__ __forceinline__ double md_dot3(double ux, double uy, double uz, double vx, double vy, double vz) { return (ux * vx + uy * vy) + uz * vz; }
__device__ __forceinline__ double md_sq3(double x, double y, double z) { return (x * x + y * y) + z * z; }

// the constants of an element in the distance pass
template <int N>
struct MdElem;
template <>
struct MdElem<3> {
    double ax, ay, az, bx, by, bz, cx, cy, cz, abx, aby, abz, acx, acy, acz, bcx, bcy, bcz;
    __device__ __forceinline__ void set(const double v[3][3]) {
        ax = v[0][0]; ay = v[0][1]; az = v[0][2];
        bx = v[1][0]; by = v[1][1]; bz = v[1][2];
        cx = v[2][0]; cy = v[2][1]; cz = v[2][2];
        abx = bx - ax; aby = by - ay; abz = bz - az;
        acx = cx - ax; acy = cy - ay; acz = cz - az;
        bcx = cx - bx; bcy = cy - by; bcz = cz - bz;
    }
    // squared distance of p to the triangle: Ericson, Real-Time Collision Detection §5.1.5, regions in his order
    __device__ __forceinline__ double dist2(const double p[3]) const {
        const double px = p[0], py = p[1], pz = p[2];
        const double apx = px - ax, apy = py - ay, apz = pz - az;
        const double d1 = md_dot3(abx, aby, abz, apx, apy, apz), d2 = md_dot3(acx, acy, acz, apx, apy, apz);
        if (d1 <= 0.0 && d2 <= 0.0) return md_sq3(apx, apy, apz);                                   // vertex a
        const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
        const double d3 = md_dot3(abx, aby, abz, bpx, bpy, bpz), d4 = md_dot3(acx, acy, acz, bpx, bpy, bpz);
        if (d3 >= 0.0 && d4 <= d3) return md_sq3(bpx, bpy, bpz);                                    // vertex b
        const double vc = d1 * d4 - d3 * d2;
        if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                                                  // edge ab
            const double v = d1 / (d1 - d3);
            return md_sq3(px - (ax + v * abx), py - (ay + v * aby), pz - (az + v * abz));
        }
        const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
        const double d5 = md_dot3(abx, aby, abz, cpx, cpy, cpz), d6 = md_dot3(acx, acy, acz, cpx, cpy, cpz);
        if (d6 >= 0.0 && d5 <= d6) return md_sq3(cpx, cpy, cpz);                                    // vertex c
        const double vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                                                  // edge ac
            const double w = d2 / (d2 - d6);
            return md_sq3(px - (ax + w * acx), py - (ay + w * acy), pz - (az + w * acz));
        }
        const double va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
        if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {                                                // edge bc
            const double w = e43 / (e43 + e56);
            return md_sq3(px - (bx + w * bcx), py - (by + w * bcy), pz - (bz + w * bcz));
        }
        const double den = (va + vb) + vc, v = vb / den, w = vc / den;                              // interior
        return md_sq3(px - ((ax + v * abx) + w * acx), py - ((ay + v * aby) + w * acy), pz - ((az + v * abz) + w * acz));
    }
};
template <>
struct MdElem<2> {
    double ax, ay, bx, by, abx, aby, den;
    __device__ __forceinline__ void set(const double v[2][2]) {
        ax = v[0][0]; ay = v[0][1];
        bx = v[1][0]; by = v[1][1];
        abx = bx - ax; aby = by - ay;
        den = abx * abx + aby * aby;
    }
    __device__ __forceinline__ double dist2(const double p[3]) const {
        const double px = p[0], py = p[1];
        const double apx = px - ax, apy = py - ay;
        const double t = abx * apx + aby * apy;
        if (t <= 0.0) return apx * apx + apy * apy;
        double rx, ry;
        if (t >= den) { rx = px - bx; ry = py - by; }
        else { const double u = t / den; rx = px - (ax + u * abx); ry = py - (ay + u * aby); }
        return rx * rx + ry * ry;
    }
};

// workgroup (one wave) = (element e0 + blockIdx.x / maxp, piece blockIdx.x % maxp of its box): lanes stride over the piece's nodes,
// axis 0 fastest.  The box is clipped to the grid and the piece to the box: every index is a grid node's.
template <int N>
__global__ void __launch_bounds__(64) md_dist_kernel(MdArgs a, unsigned long long* __restrict__ d2, long long e0, unsigned maxp) {
    const long long e = e0 + blockIdx.x / maxp;
    const long long piece = blockIdx.x % maxp;
    long long g[N];
    if (!md_indices<N>(a, e, g)) return;        // cannot happen: the host stops after md_prep
    double v[N][N];
    md_vertices<N>(a, g, v);
    int lo[3], hi[3];
    const long long vol = md_box<N>(a, v, lo, hi);
    const long long q0 = piece * MD_PIECE;
    if (q0 >= vol) return;
    const long long qend = q0 + MD_PIECE < vol ? q0 + MD_PIECE : vol;
    MdElem<N> el;
    el.set(v);
    const int bx = hi[0] - lo[0] + 1, by = hi[1] - lo[1] + 1;
    long long q = q0 + threadIdx.x;
    int i = (int)(q % bx), j, k;
    {
        const long long r = q / bx;
        j = N > 2 ? (int)(r % by) : (int)r;
        k = N > 2 ? (int)(r / by) : 0;
    }
    for (; q < qend; q += 64) {
        const int I[3] = {lo[0] + i, lo[1] + j, lo[2] + k};
        double p[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < N; ++d) p[d] = a.lc[d] + (double)I[d] * a.h[d];
        const double dd = el.dist2(p);
        const long long idx = I[0] + (long long)a.n[0] * (I[1] + (N > 2 ? (long long)a.n[1] * I[2] : 0LL));
        if (dd < __longlong_as_double((long long)d2[idx])) atomicMin(&d2[idx], (unsigned long long)__double_as_longlong(dd));
        i += 64;
        if (i >= bx) {
            const int t = i / bx;
            i -= t * bx;
            j += t;
            if (N > 2 && j >= by) { const int u = j / by; j -= u * by; k += u; }
        }
    }
}

// the first node with x_i >= xi: 0 left of the grid, n0 right of it
__device__ __forceinline__ int md_slot(const MdArgs& a, double xi) {
    const double t = (xi - a.lc[0]) / a.h[0];
    int i0 = !(t > 0.0) ? 0 : (!(t < (double)a.n[0]) ? a.n[0] : (int)ceil(t));
    while (i0 > 0 && a.lc[0] + (double)(i0 - 1) * a.h[0] >= xi) --i0;
    while (i0 < a.n[0] && a.lc[0] + (double)i0 * a.h[0] < xi) ++i0;
    return i0;
}

// MD_SUB lanes per element, striding over the grid lines of its projection
template <int N>
__global__ void __launch_bounds__(256) md_sign_kernel(MdArgs a, int* __restrict__ flips, unsigned long long* st) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long e = gid / MD_SUB;
    const int sub = (int)(gid % MD_SUB);
    if (e >= a.ne) return;
    long long g[N];
    if (!md_indices<N>(a, e, g)) return;        // cannot happen: the host stops after md_prep
    double v[N][N];
    md_vertices<N>(a, g, v);
    const long long slots = (long long)a.n[0] + 1;
    if constexpr (N == 2) {
        const double ax = v[0][0], ay = v[0][1], bx = v[1][0], by = v[1][1];
        if (ay == by) { if (sub == 0) atomicAdd(&st[MD_SKIPPED], 1ULL); return; }
        const int msig = by > ay ? -1 : 1;      // −σ
        int jlo, jhi;
        md_range(fmin(ay, by), fmax(ay, by), a.lc[1], a.h[1], a.n[1], jlo, jhi);
        for (int j = jlo + sub; j <= jhi; j += MD_SUB) {
            const double y = a.lc[1] + (double)j * a.h[1];
            if ((ay > y) == (by > y)) continue;
            const double xi = ax + ((y - ay) / (by - ay)) * (bx - ax);
            atomicAdd(&flips[j * slots + md_slot(a, xi)], msig);
        }
    } else {
    const double A2 = (v[1][1] - v[0][1]) * (v[2][2] - v[0][2]) - (v[1][2] - v[0][2]) * (v[2][1] - v[0][1]);
    if (A2 == 0.0) { if (sub == 0) atomicAdd(&st[MD_SKIPPED], 1ULL); return; }
    const int msig = A2 > 0.0 ? -1 : 1;         // −σ
    // counter-clockwise in (y, z): vertices 0, s1, s2
    const int o[3] = {0, A2 < 0.0 ? 2 : 1, A2 < 0.0 ? 1 : 2};
    double X[3], Y[3], Z[3];
    long long G[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { X[i] = v[o[i]][0]; Y[i] = v[o[i]][1]; Z[i] = v[o[i]][2]; G[i] = g[o[i]]; }
    double loy[3], loz[3], dy[3], dz[3];
    bool fwd[3], topleft[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int k = (i + 1) % 3;
        fwd[i] = G[i] < G[k];
        loy[i] = fwd[i] ? Y[i] : Y[k];
        loz[i] = fwd[i] ? Z[i] : Z[k];
        dy[i] = (fwd[i] ? Y[k] : Y[i]) - loy[i];
        dz[i] = (fwd[i] ? Z[k] : Z[i]) - loz[i];
        topleft[i] = Z[k] < Z[i] || (Z[k] == Z[i] && Y[k] < Y[i]);
    }
    int jlo, jhi, klo, khi;
    md_range(fmin(Y[0], fmin(Y[1], Y[2])), fmax(Y[0], fmax(Y[1], Y[2])), a.lc[1], a.h[1], a.n[1], jlo, jhi);
    md_range(fmin(Z[0], fmin(Z[1], Z[2])), fmax(Z[0], fmax(Z[1], Z[2])), a.lc[2], a.h[2], a.n[2], klo, khi);
    if (jhi < jlo || khi < klo) return;
    const int nj = jhi - jlo + 1;
    const long long nl = (long long)nj * (khi - klo + 1);
    for (long long l = sub; l < nl; l += MD_SUB) {
        const int j = jlo + (int)(l % nj), k = klo + (int)(l / nj);
        const double py = a.lc[1] + (double)j * a.h[1], pz = a.lc[2] + (double)k * a.h[2];
        double E[3];
        bool hit = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double Ec = dy[i] * (pz - loz[i]) - dz[i] * (py - loy[i]);
            E[i] = fwd[i] ? Ec : -Ec;
            hit = hit && (E[i] > 0.0 || (E[i] == 0.0 && topleft[i]));
        }
        if (!hit) continue;
        const double w0 = E[1], w1 = E[2], w2 = E[0];
        const double xi = ((w0 * X[0] + w1 * X[1]) + w2 * X[2]) / ((w0 + w1) + w2);
        atomicAdd(&flips[(j + (long long)a.n[1] * k) * slots + md_slot(a, xi)], msig);
    }
    }
}

// one wave per grid row (axis 0 contiguous): the winding count as a running prefix sum of the row's flip counters, 64 nodes at a time
template <int N>
__global__ void __launch_bounds__(256) md_final_kernel(MdArgs a, const unsigned long long* __restrict__ d2, const int* __restrict__ flips, void* phi,
                                                       int f32, unsigned long long* st) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.nrow) return;
    const long long j = N > 2 ? row % a.n[1] : row, k = N > 2 ? row / a.n[1] : 0;
    const long long bphi = a.origin + j * a.s1 + k * a.s2, bd = row * a.n[0], bf = row * ((long long)a.n[0] + 1);
    int carry = 0;
    unsigned near = 0;
    for (int i0 = 0; i0 < a.n[0]; i0 += 64) {
        const int i = i0 + lane;
        const int s = wave_incl_scan(i < a.n[0] ? flips[bf + i] : 0);
        if (i < a.n[0]) {
            const unsigned long long bits = d2[bd + i];
            near += bits < a.c2bits;
            const double val = sqrt(__longlong_as_double((long long)bits));
            st_val(phi, bphi + i, f32, carry + s != 0 ? -val : val);
        }
        carry += __shfl(s, 63, 64);
    }
    const int total = carry + flips[bf + a.n[0]];
    near = wave_sum(near);
    if (lane == 0) {
        if (near) atomicAdd(&st[MD_NEAR], (unsigned long long)near);
        if (total != 0) atomicAdd(&st[MD_UNBALANCED], 1ULL);
    }
}

// ---- host side
struct MdistWorkspace {
    DevBuf<unsigned long long> d2;   // bit patterns of min(d², c²), one per node
    DevBuf<int> flips;               // n0 + 1 flip counters per row; the last holds the crossings right of the grid
    DevBuf<unsigned long long> st;   // MD_NSTAT counters
};
void mdist_workspace_free(MdistWorkspace* w) { delete w; }

int mdist_run(int ndim, const int n[3], long long s1, long long s2, long long origin, const double lc[3], const double h[3], long long nv,
              const double* verts, long long ne, const long long* elems, double cutoff, void* phi, int f32, hipStream_t stream, long long stats[3],
              const char** err, MdistWorkspace** workspace) {
    if (ndim != 2 && ndim != 3) { *err = "mesh_distance: 2-D and 3-D fields only"; return 1; }
    MdArgs a;
    a.nnode = 1;
    for (int d = 0; d < 3; ++d) {
        a.n[d] = d < ndim ? n[d] : 1;
        a.lc[d] = d < ndim ? lc[d] : 0.0;
        a.h[d] = d < ndim ? h[d] : 1.0;
        if (d < ndim && n[d] < 2) { *err = "mesh_distance: at least two nodes per dimension"; return 1; }
        a.nnode *= a.n[d];
    }
    a.nrow = a.nnode / a.n[0];
    a.s1 = s1; a.s2 = ndim > 2 ? s2 : 0; a.origin = origin;
    a.c = cutoff;
    const double c2 = cutoff * cutoff;
    static_assert(sizeof(c2) == sizeof(a.c2bits), "fp64");
    memcpy(&a.c2bits, &c2, sizeof(c2));
    a.nv = nv; a.ne = ne; a.verts = verts; a.elems = elems;
    if (a.nnode > MD_MAX_BLOCKS * 256 || ne > (MD_MAX_BLOCKS * 256) / MD_SUB || nv > MD_MAX_BLOCKS * 256) {
        *err = "mesh_distance: the grid or the mesh is too large for one launch";
        return 1;
    }

    if (!*workspace) *workspace = new MdistWorkspace();     // the handle's, created by its first call; the buffers only grow
    MdistWorkspace& W = **workspace;
    const size_t nflip = (size_t)a.nrow * ((size_t)a.n[0] + 1);
    MOD_HIP(W.d2.grow((size_t)a.nnode * sizeof(unsigned long long)), "hipMalloc(squared distances)");
    MOD_HIP(W.flips.grow(nflip * sizeof(int)), "hipMalloc(flip counters)");
    MOD_HIP(W.st.grow(MD_NSTAT * sizeof(unsigned long long)), "hipMalloc(statistics)");
    MOD_HIP(hipMemsetAsync(W.st.p, 0, MD_NSTAT * sizeof(unsigned long long), stream), "mesh_distance: memset");
    MOD_HIP(hipMemsetAsync(W.flips.p, 0, nflip * sizeof(int), stream), "mesh_distance: memset");
    hipLaunchKernelGGL(md_init_kernel, dim3((unsigned)((a.nnode + 255) / 256)), dim3(256), 0, stream, W.d2.p, a.nnode, a.c2bits);
    unsigned long long st[MD_NSTAT] = {};
    if (ne > 0 || nv > 0) {
        const long long nt = std::max(ne, nv);
        LSM_LAUNCH_ND(ndim, md_prep_kernel, (unsigned)((nt + 255) / 256), 256, stream, a, W.st.p);
        MOD_HIP(hipMemcpyAsync(st, W.st.p, sizeof(st), hipMemcpyDeviceToHost, stream), "mesh_distance: validation");
        MOD_HIP(hipStreamSynchronize(stream), "mesh_distance: validation");
        if (st[MD_BAD_INDEX]) { *err = "mesh_distance: an element refers to a vertex number outside 0..nverts-1"; return 1; }
        if (st[MD_NONFINITE]) { *err = "mesh_distance: the vertices must be finite"; return 1; }
    }
    const long long maxp = (long long)st[MD_MAXPIECES];
    if (ne > 0 && maxp > 0) {
        const long long per = std::max(1LL, MD_MAX_BLOCKS / maxp);      // elements per launch
        for (long long e0 = 0; e0 < ne; e0 += per) {
            const long long cnt = std::min(per, ne - e0);
            LSM_LAUNCH_ND(ndim, md_dist_kernel, (unsigned)(cnt * maxp), 64, stream, a, W.d2.p, e0, (unsigned)maxp);
        }
    }
    if (ne > 0) LSM_LAUNCH_ND(ndim, md_sign_kernel, (unsigned)((ne * MD_SUB + 255) / 256), 256, stream, a, W.flips.p, W.st.p);
    LSM_LAUNCH_ND(ndim, md_final_kernel, (unsigned)((a.nrow + 3) / 4), 256, stream, a, W.d2.p, W.flips.p, phi, f32, W.st.p);
    MOD_HIP(hipGetLastError(), "mesh_distance: launch failed");
    MOD_HIP(hipMemcpyAsync(st, W.st.p, sizeof(st), hipMemcpyDeviceToHost, stream), "mesh_distance: statistics");
    MOD_HIP(hipStreamSynchronize(stream), "mesh_distance: device error");
    stats[0] = (long long)st[MD_NEAR];
    stats[1] = (long long)st[MD_UNBALANCED];
    stats[2] = (long long)st[MD_SKIPPED];
    return 0;
}

}  // namespace lsm
