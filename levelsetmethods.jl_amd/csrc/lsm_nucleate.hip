// lsm_nucleate.hip — hole nucleation on the device: the centres a criterion field t selects on ϕ's grid, and the punch that
// removes a ball around each.  include/lsm.h ("nucleation") is the normative text, tests/_topo_ref.py restates it, DESIGN.md
// §7.21.  The rules:
//   * candidate(I) := t_I < threshold and ϕ_I <= level − clearance, as fp64 (both false for NaN); the bound is formed once on the host;
//   * key(I) := (t_I, I), I the linear node index (axis 0 fastest), ordered lexicographically with −0 == +0; I is a centre iff it is
//     a candidate and its key is the smallest over the candidates of the box |J_d − I_d| <= w_d clipped at the grid;
//   * punch: V_I = max over the centres c with |I_d − c_d| <= B_d of level + (radius − sqrt(Σ_d ((I_d − c_d)·h_d)²)); ϕ_I := V_I where
//     ϕ_I < V_I, rounded once.
// The kernels:
//   nu_pass_x     one workgroup per 256 nodes of a row: the keys of the row segment and its w-halo in LDS (formed from t and ϕ on
//                 the way in), every thread the minimum of its 2w + 1 entries;
//   nu_pass_col   the same along y or z: a tile of 64 columns (x-contiguous: every global access is a run of 64 values) by 16
//                 lines, staged with its w-halo in dynamic LDS, (16 + 2w)·64 pairs of 12 bytes: 13.5 KB at w = 1, 60 KB at w = 32;
//   nu_count      the centres of every chunk of 4096 nodes;  chunk_scan (scan.h)  their exclusive scan in one workgroup and the
//                 total, which is the host's one read;  nu_write  (index, value) in ascending index at the scanned positions — no append whose
//                 order depends on the schedule;
//   nu_punch_mark one workgroup per centre over its clipped box: an integer atomic max of the order-preserving image of v into
//                 one 64-bit word per node;  nu_punch_apply  one thread per node: the compare with ϕ, the one store, the count.
// The minimum of a total order over a box is the minimum along x of the minimum along y of the minimum along z: the passes are
// exact, whatever their order.  A key is the order-preserving 64-bit image of t_I (nu_sortable) and the node index; a node that is
// no candidate, or lies beyond the grid, holds NU_NONE, which is above the image of every number.
#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>

#include "kuhn.h"
#include "scan.h"

namespace lsm {

constexpr unsigned long long NU_NONE = ~0ull;
constexpr unsigned NU_NOIDX = 0xffffffffu;
constexpr int NU_CHUNK = 4096;               // nodes per workgroup of the count and write kernels
constexpr int NU_PER = NU_CHUNK / 256;
constexpr int NU_TX = 64, NU_TL = 16;        // the column passes' tile: columns along x, lines along the pass's axis
constexpr int NU_WMAX = 32;

struct NuArgs {
    int n[3], w[3];
    long long s1, s2, origin;   // the padded layout of ϕ and t
    long long nnode, nchunk;
    int f32;
};
struct NuBall {
    double h[3], level, radius;
    int B[3];                   // the box's half width in nodes: floor(radius/h_d)
};

// the image of a number (not NaN) under which unsigned order is numeric order; −0 goes with +0.  Never 0 and never NU_NONE.
__device__ __forceinline__ unsigned long long nu_sortable(double v) {
    if (v == 0.0) v = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double nu_number(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ bool nu_less(unsigned long long k1, unsigned i1, unsigned long long k2, unsigned i2) {
    return k1 < k2 || (k1 == k2 && i1 < i2);
}
template <int N>
__device__ __forceinline__ long long nu_padded(const NuArgs& a, long long i) {
    const int x = (int)(i % a.n[0]);
    const long long r = i / a.n[0];
    const int y = N > 2 ? (int)(r % a.n[1]) : (int)r, z = N > 2 ? (int)(r / a.n[1]) : 0;
    return a.origin + x + y * a.s1 + z * a.s2;
}

// ---- the pass along x.  FIRST: the keys come from t and ϕ; otherwise from the pass before.  One workgroup per (row, 256 nodes).
template <int N, bool FIRST>
__global__ void __launch_bounds__(256) nu_pass_x_kernel(NuArgs a, const void* __restrict__ phi, const void* __restrict__ t, double threshold, double bound,
                                                        const unsigned long long* __restrict__ kin, const unsigned* __restrict__ iin,
                                                        unsigned long long* __restrict__ kout, unsigned* __restrict__ iout) {
    __shared__ unsigned long long sk[256 + 2 * NU_WMAX];
    __shared__ unsigned si[256 + 2 * NU_WMAX];
    const int w = a.w[0], tid = threadIdx.x;
    const int nxc = (a.n[0] + 255) / 256;
    const long long row = blockIdx.x / nxc;
    const int x0 = (int)(blockIdx.x % nxc) * 256;
    const int y = N > 2 ? (int)(row % a.n[1]) : (int)row, z = N > 2 ? (int)(row / a.n[1]) : 0;
    const long long lin0 = row * a.n[0];
    for (int e = tid; e < 256 + 2 * w; e += 256) {
        const int x = x0 - w + e;
        unsigned long long k = NU_NONE;
        unsigned i = NU_NOIDX;
        if (x >= 0 && x < a.n[0]) {
            if (FIRST) {
                const long long at = a.origin + x + y * a.s1 + z * a.s2;
                const double tv = ld_val(t, at, a.f32), pv = ld_val(phi, at, a.f32);
                i = (unsigned)(lin0 + x);
                if (tv < threshold && pv <= bound) k = nu_sortable(tv);      // false for NaN
            } else {
                k = kin[lin0 + x];
                i = iin[lin0 + x];
            }
        }
        sk[e] = k;
        si[e] = i;
    }
    __syncthreads();
    const int x = x0 + tid;
    if (x >= a.n[0]) return;
    unsigned long long bk = sk[tid];
    unsigned bi = si[tid];
    for (int e = 1; e <= 2 * w; ++e) {
        const unsigned long long k = sk[tid + e];
        const unsigned i = si[tid + e];
        if (nu_less(k, i, bk, bi)) { bk = k; bi = i; }
    }
    kout[lin0 + x] = bk;
    iout[lin0 + x] = bi;
}

// ---- the pass along AX = 1 (y) or 2 (z): one workgroup per tile of NU_TX columns by NU_TL lines (and per index of the third axis)
template <int N, int AX>
__global__ void __launch_bounds__(256) nu_pass_col_kernel(NuArgs a, const unsigned long long* __restrict__ kin, const unsigned* __restrict__ iin,
                                                          unsigned long long* __restrict__ kout, unsigned* __restrict__ iout) {
    extern __shared__ unsigned long long nu_lds[];      // (NU_TL + 2w)·NU_TX keys, then as many indices
    const int w = a.w[AX], nl = NU_TL + 2 * w;
    unsigned long long* sk = nu_lds;
    unsigned* si = reinterpret_cast<unsigned*>(sk + nl * NU_TX);
    const int nxc = (a.n[0] + NU_TX - 1) / NU_TX, nlc = (a.n[AX] + NU_TL - 1) / NU_TL;
    long long b = blockIdx.x;
    const int x0 = (int)(b % nxc) * NU_TX;
    b /= nxc;
    const int l0 = (int)(b % nlc) * NU_TL;
    const long long o = b / nlc;                        // the third axis in 3-D: z for AX = 1, y for AX = 2
    const long long sl = AX == 1 ? (long long)a.n[0] : (long long)a.n[0] * a.n[1];
    const long long so = AX == 1 ? (long long)a.n[0] * a.n[1] : (long long)a.n[0];
    const long long base = N > 2 ? o * so : 0;
    const int tx = threadIdx.x & (NU_TX - 1), ty = threadIdx.x / NU_TX;
    const int x = x0 + tx;
    for (int r = ty; r < nl; r += 256 / NU_TX) {
        const int l = l0 - w + r;
        unsigned long long k = NU_NONE;
        unsigned i = NU_NOIDX;
        if (x < a.n[0] && l >= 0 && l < a.n[AX]) {
            const long long g = base + l * sl + x;
            k = kin[g];
            i = iin[g];
        }
        sk[r * NU_TX + tx] = k;
        si[r * NU_TX + tx] = i;
    }
    __syncthreads();
    if (x >= a.n[0]) return;
    for (int r = ty; r < NU_TL; r += 256 / NU_TX) {
        const int l = l0 + r;
        if (l >= a.n[AX]) break;
        unsigned long long bk = sk[r * NU_TX + tx];
        unsigned bi = si[r * NU_TX + tx];
        for (int e = 1; e <= 2 * w; ++e) {
            const unsigned long long k = sk[(r + e) * NU_TX + tx];
            const unsigned i = si[(r + e) * NU_TX + tx];
            if (nu_less(k, i, bk, bi)) { bk = k; bi = i; }
        }
        const long long g = base + l * sl + x;
        kout[g] = bk;
        iout[g] = bi;
    }
}

// I is a centre iff the smallest key of its window is its own (then it is a candidate: NU_NONE is nobody's key)
__device__ __forceinline__ bool nu_centre(const unsigned long long* __restrict__ k, const unsigned* __restrict__ idx, long long i) {
    return k[i] != NU_NONE && idx[i] == (unsigned)i;
}

__global__ void __launch_bounds__(256) nu_count_kernel(NuArgs a, const unsigned long long* __restrict__ k, const unsigned* __restrict__ idx, unsigned* __restrict__ sums) {
    __shared__ unsigned wsum[4];
    const long long c0 = (long long)blockIdx.x * NU_CHUNK;
    unsigned c = 0;
    for (int q = 0; q < NU_PER; ++q) {
        const long long i = c0 + 256 * q + threadIdx.x;
        if (i < a.nnode && nu_centre(k, idx, i)) ++c;
    }
    c = block_sum<4>(c, wsum);
    if (threadIdx.x == 0) sums[blockIdx.x] = c;
}

template <int N>
__global__ void __launch_bounds__(256) nu_write_kernel(NuArgs a, const unsigned long long* __restrict__ k, const unsigned* __restrict__ idx, const void* __restrict__ t,
                                                       const unsigned long long* __restrict__ off, long long* __restrict__ out_i, double* __restrict__ out_v) {
    __shared__ unsigned wsum[4];
    const long long c0 = (long long)blockIdx.x * NU_CHUNK;
    unsigned long long base = off[blockIdx.x];
    for (int q = 0; q < NU_PER; ++q) {      // uniform over the workgroup: the barriers are reached by every thread
        const long long i = c0 + 256 * q + threadIdx.x;
        const bool c = i < a.nnode && nu_centre(k, idx, i);
        unsigned tot;
        const unsigned ex = block_excl_scan<4>(c ? 1u : 0u, wsum, tot);
        if (c) {
            out_i[base + ex] = i;
            out_v[base + ex] = ld_val(t, nu_padded<N>(a, i), a.f32);
        }
        base += tot;
        __syncthreads();      // wsum is written again
    }
}

// the workgroup's number of set flags added to *dst by one atomic.  Every thread calls this.
__device__ __forceinline__ void nu_block_add(bool flag, unsigned* s_tot, unsigned long long* dst) {
    if (threadIdx.x == 0) *s_tot = 0;
    __syncthreads();
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(s_tot, (unsigned)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && *s_tot) atomicAdd(dst, (unsigned long long)*s_tot);
}

// ---- punch, first pass: vmax[I] := max(vmax[I], image of v) over the centre's clipped box.  vmax is 0 where no box reaches.  A
// centre outside the grid is counted in cnt[0] and writes nothing.
template <int N>
__global__ void __launch_bounds__(256) nu_punch_mark_kernel(NuArgs a, NuBall b, const long long* __restrict__ centres, unsigned long long* vmax, unsigned long long* cnt) {
    const long long c = centres[blockIdx.x];
    if (c < 0 || c >= a.nnode) {
        if (threadIdx.x == 0) atomicAdd(&cnt[0], 1ull);
        return;
    }
    int cI[3], lo[3], ext[3];
    cI[0] = (int)(c % a.n[0]);
    const long long r = c / a.n[0];
    cI[1] = N > 2 ? (int)(r % a.n[1]) : (int)r;
    cI[2] = N > 2 ? (int)(r / a.n[1]) : 0;
    long long total = 1;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        lo[d] = d < N ? max(0, cI[d] - b.B[d]) : 0;
        const int hi = d < N ? min(a.n[d] - 1, cI[d] + b.B[d]) : 0;
        ext[d] = hi - lo[d] + 1;
        total *= ext[d];
    }
    for (long long e = threadIdx.x; e < total; e += 256) {
        int I[3];
        I[0] = lo[0] + (int)(e % ext[0]);
        const long long q = e / ext[0];
        I[1] = lo[1] + (N > 2 ? (int)(q % ext[1]) : (int)q);
        I[2] = N > 2 ? lo[2] + (int)(q / ext[1]) : 0;
        double d2 = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const double x = (double)(I[d] - cI[d]) * b.h[d];
            d2 = d2 + x * x;
        }
        const double v = b.level + (b.radius - sqrt(d2));
        atomicMax(&vmax[I[0] + (long long)a.n[0] * (I[1] + (long long)a.n[1] * I[2])], nu_sortable(v));
    }
}

// ---- punch, second pass: ϕ_I := V_I where ϕ_I < V_I (false for a NaN ϕ), rounded once; cnt[1] += the stored values whose bits changed
template <int N>
__global__ void __launch_bounds__(256) nu_punch_apply_kernel(NuArgs a, void* phi, const unsigned long long* __restrict__ vmax, unsigned long long* cnt) {
    __shared__ unsigned s_tot;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool changed = false;
    if (i < a.nnode) {
        const unsigned long long k = vmax[i];
        if (k) {
            const double v = nu_number(k);
            const long long at = nu_padded<N>(a, i);
            if (a.f32) {
                float* p = static_cast<float*>(phi) + at;
                const float old = *p;
                if ((double)old < v) {
                    const float f = (float)v;
                    if (__float_as_int(f) != __float_as_int(old)) {
                        *p = f;
                        changed = true;
                    }
                }
            } else {
                double* p = static_cast<double*>(phi) + at;
                if (*p < v) {
                    *p = v;
                    changed = true;
                }
            }
        }
    }
    nu_block_add(changed, &s_tot, &cnt[1]);
}

// ---- host side
struct NuWorkspace {
    DevBuf<unsigned long long> ka, kb;      // a key per node, twice (the passes go to and fro); ka is the punch's vmax
    DevBuf<unsigned> ia, ib;                // the index that goes with it
    DevBuf<unsigned> sums;                  // one per chunk
    DevBuf<unsigned long long> off;         // their exclusive scan
    DevBuf<unsigned long long> cnt;         // [0] the total of the scan; [1], [2] the punch's counters
};
void nu_workspace_free(NuWorkspace* w) { delete w; }

struct NuObject {
    long long count = 0;
    DevBuf<long long> idx;
    DevBuf<double> val;
    hipStream_t stream = nullptr;
};

static int nu_args(const LsmHandle* h, NuArgs& a, const char** err) {
    const int ndim = h->grid.ndim;
    if (ndim != 2 && ndim != 3) { *err = "nucleate: 2-D and 3-D fields only"; return 1; }
    a.nnode = 1;
    for (int d = 0; d < 3; ++d) {
        a.n[d] = d < ndim ? h->nloc[d] : 1;
        a.w[d] = 0;
        if (a.n[d] < 1) { *err = "nucleate: an empty grid"; return 1; }
        if (a.nnode > (long long)INT_MAX / a.n[d]) { *err = "nucleate: the grid has 2^31 - 1 nodes or more"; return 1; }
        a.nnode *= a.n[d];
    }
    if (a.nnode >= (long long)INT_MAX) { *err = "nucleate: the grid has 2^31 - 1 nodes or more"; return 1; }
    a.s1 = h->lay.stride[1]; a.s2 = ndim > 2 ? h->lay.stride[2] : 0; a.origin = h->lay.origin;
    a.nchunk = (a.nnode + NU_CHUNK - 1) / NU_CHUNK;
    a.f32 = h->dtype == LSM_DTYPE_F32;
    return 0;
}

static int nu_grow(NuWorkspace** workspace, const NuArgs& a, bool search, const char** err) {
    if (!*workspace) *workspace = new NuWorkspace();      // the handle's, created by its first call; the buffers only grow
    NuWorkspace& W = **workspace;
    MOD_HIP(W.ka.grow((size_t)a.nnode * sizeof(unsigned long long)), "hipMalloc(keys)");
    MOD_HIP(W.cnt.grow(3 * sizeof(unsigned long long)), "hipMalloc(counters)");
    if (search) {
        MOD_HIP(W.kb.grow((size_t)a.nnode * sizeof(unsigned long long)), "hipMalloc(keys)");
        MOD_HIP(W.ia.grow((size_t)a.nnode * sizeof(unsigned)), "hipMalloc(key indices)");
        MOD_HIP(W.ib.grow((size_t)a.nnode * sizeof(unsigned)), "hipMalloc(key indices)");
        MOD_HIP(W.sums.grow((size_t)a.nchunk * sizeof(unsigned)), "hipMalloc(chunk sums)");
        MOD_HIP(W.off.grow((size_t)a.nchunk * sizeof(unsigned long long)), "hipMalloc(chunk offsets)");
    }
    return 0;
}

// returns 0, 1 (refused: *err says why) or 2 (a HIP call failed)
int nu_build(const LsmHandle* h, NuWorkspace** workspace, const void* phi, const void* t, double threshold, double level, double clearance, double spacing,
             NuObject** out, long long* count, const char** err) {
    NuArgs a;
    if (const int r = nu_args(h, a, err)) return r;
    const int ndim = h->grid.ndim;
    if (!std::isfinite(threshold) || !std::isfinite(level) || !std::isfinite(clearance) || !std::isfinite(spacing)) {
        *err = "nucleate: threshold, level, clearance and spacing must be finite";
        return 1;
    }
    for (int d = 0; d < ndim; ++d) {
        const double w = std::ceil(spacing / h->h[d]);
        if (!(w >= 1.0 && w <= (double)NU_WMAX)) { *err = "nucleate: ceil(spacing/h) must lie in [1, 32] along every axis"; return 1; }
        a.w[d] = (int)w;
    }
    const double bound = level - clearance;
    const hipStream_t stream = h->stream;
    (void)hipSetDevice(h->device);
    if (const int r = nu_grow(workspace, a, true, err)) return r;
    NuWorkspace& W = **workspace;
    std::unique_ptr<NuObject> o(new NuObject());
    o->stream = stream;

    const long long rows = a.nnode / a.n[0];
    const unsigned gx = (unsigned)(rows * ((a.n[0] + 255) / 256));
    const long long nxc = (a.n[0] + NU_TX - 1) / NU_TX;
    const unsigned long long *kn = nullptr;
    const unsigned* in = nullptr;
    if (ndim == 2) {
        hipLaunchKernelGGL((nu_pass_x_kernel<2, true>), dim3(gx), dim3(256), 0, stream, a, phi, t, threshold, bound, kn, in, W.ka.p, W.ia.p);
        const unsigned gy = (unsigned)(nxc * ((a.n[1] + NU_TL - 1) / NU_TL));
        const size_t lds = (size_t)(NU_TL + 2 * a.w[1]) * NU_TX * 12;
        hipLaunchKernelGGL((nu_pass_col_kernel<2, 1>), dim3(gy), dim3(256), lds, stream, a, (const unsigned long long*)W.ka.p, (const unsigned*)W.ia.p, W.kb.p, W.ib.p);
    } else {
        hipLaunchKernelGGL((nu_pass_x_kernel<3, true>), dim3(gx), dim3(256), 0, stream, a, phi, t, threshold, bound, kn, in, W.ka.p, W.ia.p);
        const unsigned gy = (unsigned)(nxc * ((a.n[1] + NU_TL - 1) / NU_TL) * a.n[2]);
        const size_t ldy = (size_t)(NU_TL + 2 * a.w[1]) * NU_TX * 12;
        hipLaunchKernelGGL((nu_pass_col_kernel<3, 1>), dim3(gy), dim3(256), ldy, stream, a, (const unsigned long long*)W.ka.p, (const unsigned*)W.ia.p, W.kb.p, W.ib.p);
        const unsigned gz = (unsigned)(nxc * ((a.n[2] + NU_TL - 1) / NU_TL) * a.n[1]);
        const size_t ldz = (size_t)(NU_TL + 2 * a.w[2]) * NU_TX * 12;
        hipLaunchKernelGGL((nu_pass_col_kernel<3, 2>), dim3(gz), dim3(256), ldz, stream, a, (const unsigned long long*)W.kb.p, (const unsigned*)W.ib.p, W.ka.p, W.ia.p);
    }
    const unsigned long long* kf = ndim == 2 ? W.kb.p : W.ka.p;      // where the last pass left the minima
    const unsigned* xf = ndim == 2 ? W.ib.p : W.ia.p;
    const unsigned nchunk = (unsigned)a.nchunk;
    hipLaunchKernelGGL(nu_count_kernel, dim3(nchunk), dim3(256), 0, stream, a, kf, xf, W.sums.p);
    chunk_scan<1, unsigned long long>(stream, {{{W.sums.p, W.off.p, 0}}}, a.nchunk, W.cnt.p);
    MOD_HIP(hipGetLastError(), "nucleate: launch failed");
    unsigned long long total = 0;
    MOD_HIP(hipMemcpyAsync(&total, W.cnt.p, sizeof(total), hipMemcpyDeviceToHost, stream), "nucleate: count");
    MOD_HIP(hipStreamSynchronize(stream), "nucleate: device error");
    if (total > (unsigned long long)a.nnode) { *err = "nucleate: more centres than nodes"; return 2; }
    o->count = (long long)total;
    MOD_HIP(o->idx.alloc((size_t)std::max(o->count, 1LL) * sizeof(long long)), "hipMalloc(centres)");
    MOD_HIP(o->val.alloc((size_t)std::max(o->count, 1LL) * sizeof(double)), "hipMalloc(centre values)");
    if (o->count) {
        LSM_LAUNCH_ND(ndim, nu_write_kernel, nchunk, 256, stream, a, kf, xf, t, (const unsigned long long*)W.off.p, o->idx.p, o->val.p);
        MOD_HIP(hipGetLastError(), "nucleate: launch failed");
        MOD_HIP(hipStreamSynchronize(stream), "nucleate: device error");
    }
    *count = o->count;
    *out = o.release();
    return 0;
}

int nu_read(NuObject* o, long long* indices, double* values, const char** err) {
    const size_t K = (size_t)o->count;
    return kuhn_read(o->stream, {{indices, o->idx, K * sizeof(long long)}, {values, o->val, K * sizeof(double)}}, "nucleate read: device error", err);
}

void nu_free(NuObject* o) { delete o; }

// returns 0, 1 (refused: phi untouched) or 2 (a HIP call failed)
int nu_punch(const LsmHandle* h, NuWorkspace** workspace, void* phi, const long long* centres, long long count, double level, double radius, long long* changed,
             const char** err) {
    NuArgs a;
    *changed = 0;
    if (const int r = nu_args(h, a, err)) return r;
    const int ndim = h->grid.ndim;
    if (!std::isfinite(level) || !std::isfinite(radius) || !(radius > 0.0)) { *err = "nucleate punch: level must be finite, radius finite and positive"; return 1; }
    if (count < 0 || count >= (long long)INT_MAX) { *err = "nucleate punch: the number of centres must lie in [0, 2^31 - 1)"; return 1; }
    if (!count) return 0;
    NuBall b;
    b.level = level; b.radius = radius;
    for (int d = 0; d < 3; ++d) {
        b.h[d] = d < ndim ? h->h[d] : 1.0;
        b.B[d] = d < ndim ? (int)std::min(std::floor(radius / h->h[d]), (double)a.n[d]) : 0;
    }
    const hipStream_t stream = h->stream;
    (void)hipSetDevice(h->device);
    if (const int r = nu_grow(workspace, a, false, err)) return r;
    NuWorkspace& W = **workspace;
    unsigned long long* cnt = W.cnt.p + 1;
    MOD_HIP(hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned long long), stream), "nucleate punch: memset");
    MOD_HIP(hipMemsetAsync(W.ka.p, 0, (size_t)a.nnode * sizeof(unsigned long long), stream), "nucleate punch: memset");
    LSM_LAUNCH_ND(ndim, nu_punch_mark_kernel, (unsigned)count, 256, stream, a, b, centres, W.ka.p, cnt);
    MOD_HIP(hipGetLastError(), "nucleate punch: launch failed");
    unsigned long long c[2] = {};
    MOD_HIP(hipMemcpyAsync(c, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream), "nucleate punch: counts");
    MOD_HIP(hipStreamSynchronize(stream), "nucleate punch: device error");
    if (c[0]) { *err = "nucleate punch: a centre is not a node index of the grid"; return 1; }
    const unsigned nblk = (unsigned)((a.nnode + 255) / 256);
    LSM_LAUNCH_ND(ndim, nu_punch_apply_kernel, nblk, 256, stream, a, phi, (const unsigned long long*)W.ka.p, cnt);
    MOD_HIP(hipGetLastError(), "nucleate punch: launch failed");
    MOD_HIP(hipMemcpyAsync(c, cnt, sizeof(c), hipMemcpyDeviceToHost, stream), "nucleate punch: counts");
    MOD_HIP(hipStreamSynchronize(stream), "nucleate punch: device error");
    *changed = (long long)c[1];
    return 0;
}

}  // namespace lsm
