// lsm_semilag.hip — SemiLagrangian: one large advection step by backward characteristics.  Every node is traced
// back along the velocity for Δt and ϕⁿ is read at the departure point by a tensor-product Lagrange interpolant: one gather pass,
// unconditionally stable.  The reference has no such integrator; the scheme is this library's and DESIGN.md fixes every operation
// order (tests/_semilag_ref.py restates it in numpy, and the device equals it bit for bit).
//
// Index space.  i_d is the node index as a double, n_d the node count, p_d = n_d − 1.
//   trace = 1   ξ_d = W(i_d − (Δt·u_d(node, tc))/h_d)
//   trace = 2   t_h = tc + ½Δt,  ξᵐ_d = W(i_d − ((½Δt)·u_d(node, t_h))/h_d),  ξ_d = W(i_d − (Δt·u_d(ξᵐ, t_h))/h_d)
//   W           periodic axis: ξ − floor(ξ/p)·p;  every other axis: ξ < 0 → 0, ξ > p → p (NaN stays NaN)
//   cell        f = floor(ξ); j = f if 0 ≤ f ≤ n − 2, n − 2 if f > n − 2, else 0 (NaN and negatives: 0; the conversion only sees values in
//               range, and the integer is clamped once more); θ = ξ − j
//   velocity    at a node: the node value.  Off the nodes: CONST the constant; ROTATION the formula of include/lsm.h at x = lc + ξ·h;
//               SEPARABLE ((L₁·L₂)·L₃)·g(t) with L_e = a + θ_e·(b − a) of table entries j_e, j_e + 1; FIELD a + θ·(b − a) along
//               dimension 1, then 2, then 3 over the 2ᴺ nodes of the cell (in-grid nodes only: coefficient fields have no ghosts)
//   weights     nodes s = −r+1 … r (r = 1, 2, 3 for order 1, 3, 5): w_s = (Π_{m≠s}(θ − m), m ascending, from 1.0) / Π_{m≠s}(s − m)
//   interpolant dimension 1 first: every x-line Σ_s w_s·ϕ (s ascending, starting from the first product), then the lines along
//               dimension 2, then 3.  Stencil nodes outside the grid are ϕ's ghost layers (filled on entry, all dimensions).
//   limiter     lo / hi over the 2ᴺ corners of the cell in stencil order (dimension 3 outermost), `v < lo ? v : lo`; the result is
//               `x < lo ? lo : (x > hi ? hi : x)`: a NaN result stays NaN
// Float32 storage widens on load and rounds once on store.  This object is compiled without contraction: FAST and STRICT handles
// run the same code.
//
// Two kernels with the same per-node code (sl_trace, sl_interp):
//   direct   one thread per node, x fastest; every stencil value comes from global memory.  Correct for any displacement; the default
//            (it is the faster one for orders 1 and 3: DESIGN.md §7.30).
//   staged   a workgroup owns a tile of TX × TY × TZ nodes, SL_K per thread.  It traces them, reduces the bounding box of their cells
//            (wave.h's min / max), and when the box plus the stencil halo fits SL_LDS doubles it copies the box into LDS by coalesced
//            rows and interpolates from there; otherwise the workgroup reads global memory like the direct kernel.  The decision is
//            uniform per workgroup.  SL_LDS·8 B = 62 KiB: two workgroups stay resident on a CU (160 KiB).  LSM_SEMILAG_STAGE = 1.
// Counters (staged / other workgroups, largest displacement) cost nothing unless asked for: then every workgroup stores one record
// of its own and semilag_stats_kernel reduces them — no atomics.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lsm_handle.h"
#include "wave.h"

namespace lsm {

static const int SL_THREADS = 256;
static const int SL_K = 4;            // nodes per thread of the staged kernel
static const int SL_LDS = 7936;       // doubles of the staged box (62 KiB)

// what a workgroup reports: a plain store of its own record, no atomics; semilag_stats_kernel reduces the records afterwards
struct SlRec { double disp; unsigned staged, _pad; };

struct SlArgs {
    int n[3];
    int per[3];                // the axis wraps (PeriodicBC on both faces)
    long long s1, s2, origin;
    double lc[3], h[3];
    double dt, hdt;            // Δt, ½Δt
    int trace, limiter, f32;
    int mode;                  // staged kernel: 1 stage where the box fits, 2 count only (nothing is written)
    CoeffArgs vel;             // tfac at tc (trace 1) or at t_h (trace 2)
    const void* phi;
    void* out;
    SlRec* rec;                // one record per workgroup, written only when the caller wants the counters (else NULL)
    int tile[3];               // staged kernel: TX, TY, TZ
};

struct SlCell { int j; double th; };

__device__ __forceinline__ double sl_wrap(double xi, int n, int per) {
    const double p = (double)(n - 1);
    if (per) return xi - floor(xi / p) * p;
    return xi < 0.0 ? 0.0 : (xi > p ? p : xi);
}

__device__ __forceinline__ SlCell sl_cell(double xi, int n) {
    const double f = floor(xi);
    const double top = (double)(n - 2);
    int j = (f >= 0.0 && f <= top) ? (int)f : (f > top ? n - 2 : 0);
    j = j < 0 ? 0 : (j > n - 2 ? n - 2 : j);
    return {j, xi - (double)j};
}

__device__ __forceinline__ double sl_lerp(double a, double b, double th) { return a + th * (b - a); }

// velocity at node I
template <int N>
__device__ __forceinline__ void sl_vel_node(const SlArgs& a, const int I[3], double u[3]) {
    const CoeffArgs& c = a.vel;
    if (c.kind == LSM_COEFF_CONST) {
        for (int d = 0; d < N; ++d) u[d] = c.v[d];
    } else if (c.kind == LSM_COEFF_ROTATION) {
        u[0] = -(c.v[0] * ((a.lc[1] + (double)I[1] * a.h[1]) - c.v[2]));
        if (N > 1) u[1] = c.v[0] * ((a.lc[0] + (double)I[0] * a.h[0]) - c.v[1]);
        if (N > 2) u[2] = 0.0;
    } else if (c.kind == LSM_COEFF_SEPARABLE) {
        for (int d = 0; d < N; ++d) {
            const double* T = c.sep[d];
            double p = T[I[0]];
            if (N > 1) p = p * T[a.n[0] + I[1]];
            if (N > 2) p = p * T[a.n[0] + a.n[1] + I[2]];
            u[d] = p * c.tfac;
        }
    } else {
        const long long q = a.origin + I[0] + I[1] * a.s1 + I[2] * a.s2;
        for (int d = 0; d < N; ++d) u[d] = c.f[d][q];
    }
}

// velocity at the point xi (index space, already mapped by W)
template <int N>
__device__ __forceinline__ void sl_vel_at(const SlArgs& a, const double xi[3], double u[3]) {
    const CoeffArgs& c = a.vel;
    if (c.kind == LSM_COEFF_CONST) {
        for (int d = 0; d < N; ++d) u[d] = c.v[d];
        return;
    }
    if (c.kind == LSM_COEFF_ROTATION) {
        u[0] = -(c.v[0] * ((a.lc[1] + (N > 1 ? xi[1] : 0.0) * a.h[1]) - c.v[2]));
        if (N > 1) u[1] = c.v[0] * ((a.lc[0] + xi[0] * a.h[0]) - c.v[1]);
        if (N > 2) u[2] = 0.0;
        return;
    }
    SlCell cl[3];
    for (int d = 0; d < N; ++d) cl[d] = sl_cell(xi[d], a.n[d]);
    if (c.kind == LSM_COEFF_SEPARABLE) {
        for (int d = 0; d < N; ++d) {
            const double* T = c.sep[d];
            double p = sl_lerp(T[cl[0].j], T[cl[0].j + 1], cl[0].th);
            if (N > 1) p = p * sl_lerp(T[a.n[0] + cl[1].j], T[a.n[0] + cl[1].j + 1], cl[1].th);
            if (N > 2) p = p * sl_lerp(T[a.n[0] + a.n[1] + cl[2].j], T[a.n[0] + a.n[1] + cl[2].j + 1], cl[2].th);
            u[d] = p * c.tfac;
        }
        return;
    }
    const long long q = a.origin + cl[0].j + (N > 1 ? cl[1].j * a.s1 : 0) + (N > 2 ? cl[2].j * a.s2 : 0);
    for (int d = 0; d < N; ++d) {
        const double* F = c.f[d] + q;
        double z[2];
#pragma unroll
        for (int kz = 0; kz < (N > 2 ? 2 : 1); ++kz) {
            double y[2];
#pragma unroll
            for (int ky = 0; ky < (N > 1 ? 2 : 1); ++ky) {
                const long long o = ky * a.s1 + kz * a.s2;
                y[ky] = sl_lerp(F[o], F[o + 1], cl[0].th);
            }
            z[kz] = N > 1 ? sl_lerp(y[0], y[1], cl[1].th) : y[0];
        }
        u[d] = N > 2 ? sl_lerp(z[0], z[1], cl[2].th) : z[0];
    }
}

// the departure cell of node I; returns the largest |Δt·u_d/h_d| of the final trace (NaN dropped)
template <int N>
__device__ __forceinline__ double sl_trace(const SlArgs& a, const int I[3], SlCell cl[3]) {
    double u[3];
    sl_vel_node<N>(a, I, u);
    if (a.trace == 2) {
        double xm[3];
        for (int d = 0; d < N; ++d) xm[d] = sl_wrap((double)I[d] - (a.hdt * u[d]) / a.h[d], a.n[d], a.per[d]);
        sl_vel_at<N>(a, xm, u);
    }
    double disp = 0.0;
    for (int d = 0; d < N; ++d) {
        const double s = (a.dt * u[d]) / a.h[d];
        const double m = fabs(s);
        disp = m > disp ? m : disp;
        cl[d] = sl_cell(sl_wrap((double)I[d] - s, a.n[d], a.per[d]), a.n[d]);
    }
    return disp;
}

template <int R>
__device__ __forceinline__ void sl_weights(double th, double w[2 * R]) {
#pragma unroll
    for (int s = 0; s < 2 * R; ++s) {
        double num = 1.0, den = 1.0;
#pragma unroll
        for (int m = 0; m < 2 * R; ++m) {
            if (m == s) continue;
            num = num * (th - (double)(m - R + 1));
            den = den * (double)(s - m);
        }
        w[s] = num / den;
    }
}

// the interpolant at the cell cl; rd(x, y, z) returns ϕ at an index of the padded field (ghosts included)
template <int N, int R, class Rd>
__device__ __forceinline__ double sl_interp(const SlCell cl[3], int limiter, Rd rd) {
    constexpr int S = 2 * R, SY = N > 1 ? S : 1, SZ = N > 2 ? S : 1;
    double wx[S], wy[S], wz[S];
    sl_weights<R>(cl[0].th, wx);
    if (N > 1) sl_weights<R>(cl[1].th, wy);
    if (N > 2) sl_weights<R>(cl[2].th, wz);
    const int bx = cl[0].j - R + 1, by = N > 1 ? cl[1].j - R + 1 : 0, bz = N > 2 ? cl[2].j - R + 1 : 0;
    double lo = 0.0, hi = 0.0, az = 0.0;
    bool first = true;
#pragma unroll
    for (int sz = 0; sz < SZ; ++sz) {
        double ay = 0.0;
#pragma unroll
        for (int sy = 0; sy < SY; ++sy) {
            double ax = 0.0;
#pragma unroll
            for (int sx = 0; sx < S; ++sx) {
                const double v = rd(bx + sx, by + sy, bz + sz);
                ax = sx == 0 ? wx[0] * v : ax + wx[sx] * v;
                const bool corner = (sx == R - 1 || sx == R) && (N < 2 || sy == R - 1 || sy == R) && (N < 3 || sz == R - 1 || sz == R);
                if (corner) {
                    if (first) { lo = v; hi = v; first = false; }
                    else { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
                }
            }
            if (N > 1) ay = sy == 0 ? wy[0] * ax : ay + wy[sy] * ax;
            else ay = ax;
        }
        if (N > 2) az = sz == 0 ? wz[0] * ay : az + wz[sz] * ay;
        else az = ay;
    }
    if (limiter) az = az < lo ? lo : (az > hi ? hi : az);
    return az;
}

// the workgroup's record: its largest displacement (reduced over the waves through `red`) and the path it took.  Every thread of
// the workgroup calls this, and only when a.rec is set.
__device__ __forceinline__ void sl_record(const SlArgs& a, double disp, bool staged, double* red) {
    const double m = wave_max(disp);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < SL_THREADS / 64; ++w) t = red[w] > t ? red[w] : t;
        const unsigned wg = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        a.rec[wg] = {t, staged ? 1u : 0u, 0u};
    }
}

// the counters of a launch from its records: out[0] staged workgroups, out[1] the others, out[2] the bits of the largest displacement
__global__ void __launch_bounds__(SL_THREADS) semilag_stats_kernel(const SlRec* rec, unsigned nwg, unsigned long long* out) {
    __shared__ double rmax[SL_THREADS / 64];
    __shared__ unsigned rsum[SL_THREADS / 64];
    double m = 0.0;
    unsigned st = 0;
    for (unsigned i = threadIdx.x; i < nwg; i += SL_THREADS) {
        const SlRec r = rec[i];
        m = r.disp > m ? r.disp : m;
        st += r.staged;
    }
    m = wave_max(m);
    st = wave_sum(st);
    if ((threadIdx.x & 63) == 0) { rmax[threadIdx.x >> 6] = m; rsum[threadIdx.x >> 6] = st; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < SL_THREADS / 64; ++w) { m = rmax[w] > m ? rmax[w] : m; st += rsum[w]; }
        out[0] = st;
        out[1] = nwg - st;
        out[2] = (unsigned long long)__double_as_longlong(m);
    }
}

// ---- direct gather: one thread per node, x fastest.  Workgroups of 64 × 4 nodes in x and y (256 in x in 1-D), one plane each: no
// division decodes an index
template <int N, int R>
__global__ void __launch_bounds__(SL_THREADS) semilag_direct_kernel(const SlArgs a) {
    __shared__ double red[SL_THREADS / 64];
    int I[3];
    if (N == 1) { I[0] = (int)(blockIdx.x * SL_THREADS + threadIdx.x); I[1] = 0; I[2] = 0; }
    else { I[0] = (int)(blockIdx.x * 64 + (threadIdx.x & 63)); I[1] = (int)(blockIdx.y * 4 + (threadIdx.x >> 6)); I[2] = (int)blockIdx.z; }
    double disp = 0.0;
    if (I[0] < a.n[0] && I[1] < a.n[1]) {
        SlCell cl[3];
        disp = sl_trace<N>(a, I, cl);
        const double v = sl_interp<N, R>(cl, a.limiter, [&](int x, int y, int z) { return ld_val(a.phi, a.origin + x + y * a.s1 + z * a.s2, a.f32); });
        st_val(a.out, a.origin + I[0] + I[1] * a.s1 + I[2] * a.s2, a.f32, v);
    }
    if (a.rec) sl_record(a, disp, false, red);
}

// ---- staged tile
template <int N, int R>
__global__ void __launch_bounds__(SL_THREADS) semilag_staged_kernel(const SlArgs a) {
    __shared__ double box[SL_LDS];
    __shared__ double red[6][SL_THREADS / 64];
    const int TX = a.tile[0], TY = a.tile[1];
    const int t0[3] = {(int)blockIdx.x * a.tile[0], (int)blockIdx.y * a.tile[1], (int)blockIdx.z * a.tile[2]};
    SlCell cl[SL_K][3];
    int I[SL_K][3];
    bool live[SL_K];
    double disp = 0.0;
    double bmin[3] = {1e300, 1e300, 1e300}, bmax[3] = {-1e300, -1e300, -1e300};
#pragma unroll
    for (int k = 0; k < SL_K; ++k) {
        const int q = k * SL_THREADS + (int)threadIdx.x;
        I[k][0] = t0[0] + q % TX;
        I[k][1] = t0[1] + (q / TX) % TY;
        I[k][2] = t0[2] + q / (TX * TY);
        live[k] = I[k][0] < a.n[0] && I[k][1] < a.n[1] && I[k][2] < a.n[2];
        if (!live[k]) continue;
        const double m = sl_trace<N>(a, I[k], cl[k]);
        disp = m > disp ? m : disp;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const double j = (double)cl[k][d].j;
            bmin[d] = j < bmin[d] ? j : bmin[d];
            bmax[d] = j > bmax[d] ? j : bmax[d];
        }
    }
    // the bounding box of the workgroup's cells
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        const double lo = wave_min(bmin[d]), hi = wave_max(bmax[d]);
        if (lane == 0) { red[d][wave] = lo; red[3 + d][wave] = hi; }
    }
    __syncthreads();
    int b0[3] = {0, 0, 0}, ext[3] = {1, 1, 1};
#pragma unroll
    for (int d = 0; d < N; ++d) {
        double lo = red[d][0], hi = red[3 + d][0];
#pragma unroll
        for (int w = 1; w < SL_THREADS / 64; ++w) {
            lo = red[d][w] < lo ? red[d][w] : lo;
            hi = red[3 + d][w] > hi ? red[3 + d][w] : hi;
        }
        b0[d] = (int)lo - R + 1;
        ext[d] = ((int)hi - (int)lo + 1) + 2 * R - 1;
    }
    const long long vol = (long long)ext[0] * ext[1] * ext[2];
    const bool staged = vol <= SL_LDS;   // uniform over the workgroup
    if (a.rec) {
        __syncthreads();   // red is read above and written again
        sl_record(a, disp, staged, &red[0][0]);
    }
    if (a.mode == 2) return;
    if (staged) {
        // rows of the box, coalesced along x; every index lies inside the padded field: b0 ≥ −R + 1 and b0 + ext − 1 ≤ n − 2 + R
        const int nrows = ext[1] * ext[2];
        for (int row = wave; row < nrows; row += SL_THREADS / 64) {
            const int y = row % ext[1], z = row / ext[1];
            const long long g = a.origin + b0[0] + (long long)(b0[1] + y) * a.s1 + (long long)(b0[2] + z) * a.s2;
            for (int x = lane; x < ext[0]; x += 64) box[row * ext[0] + x] = ld_val(a.phi, g + x, a.f32);
        }
        __syncthreads();
    }
    const int ex = ext[0], exy = ext[0] * ext[1];
#pragma unroll
    for (int k = 0; k < SL_K; ++k) {
        if (!live[k]) continue;
        double v;
        if (staged) v = sl_interp<N, R>(cl[k], a.limiter, [&](int x, int y, int z) { return box[(x - b0[0]) + (y - b0[1]) * ex + (z - b0[2]) * exy]; });
        else v = sl_interp<N, R>(cl[k], a.limiter, [&](int x, int y, int z) { return ld_val(a.phi, a.origin + x + y * a.s1 + z * a.s2, a.f32); });
        st_val(a.out, a.origin + I[k][0] + I[k][1] * a.s1 + I[k][2] * a.s2, a.f32, v);
    }
}

static dim3 sl_grid(int N, const SlArgs& a, bool staged) {
    if (staged) return dim3((a.n[0] + a.tile[0] - 1) / a.tile[0], (a.n[1] + a.tile[1] - 1) / a.tile[1], (a.n[2] + a.tile[2] - 1) / a.tile[2]);
    if (N == 1) return dim3((a.n[0] + SL_THREADS - 1) / SL_THREADS, 1, 1);
    return dim3((a.n[0] + 63) / 64, (a.n[1] + 3) / 4, a.n[2]);
}

template <int N, int R>
static void sl_launch(const SlArgs& a, bool staged, hipStream_t st) {
    if (staged) hipLaunchKernelGGL((semilag_staged_kernel<N, R>), sl_grid(N, a, true), dim3(SL_THREADS), 0, st, a);
    else hipLaunchKernelGGL((semilag_direct_kernel<N, R>), sl_grid(N, a, false), dim3(SL_THREADS), 0, st, a);
}

template <int N>
static void sl_launch_r(const SlArgs& a, int order, bool staged, hipStream_t st) {
    if (order == 1) sl_launch<N, 1>(a, staged, st);
    else if (order == 3) sl_launch<N, 2>(a, staged, st);
    else sl_launch<N, 3>(a, staged, st);
}

static void sl_launch_n(int N, const SlArgs& a, int order, bool staged, hipStream_t st) {
    if (N == 1) sl_launch_r<1>(a, order, staged, st);
    else if (N == 2) sl_launch_r<2>(a, order, staged, st);
    else sl_launch_r<3>(a, order, staged, st);
}

struct SemilagWorkspace {
    DevBuf<unsigned long long> stats;       // 3 words
    DevBuf<SlRec> rec;                      // one record per workgroup of the last launch that was asked for its counters (grow-only)
    PinnedBuf<unsigned long long> h_stats;
};

void semilag_workspace_free(SemilagWorkspace* w) { delete w; }

}  // namespace lsm

using namespace lsm;

int lsm_advance_semilag(LsmHandle* h, const LsmTerm* term, void* phi, void* out, double tc, double dt, int order, int trace, int limiter,
                        int64_t* stats) {
    if (!h) return LSM_ERR_INVALID;
    if (!term || !phi || !out) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: null argument");
    if (out == phi) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: the step is out of place (out == phi)");
    if (term->kind != LSM_TERM_ADVECTION) return lsm_fail(h, LSM_ERR_INVALID, "SemiLagrangian requires exactly one AdvectionTerm");
    if (order != 1 && order != 3 && order != 5) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: order must be 1, 3 or 5");
    if (trace != 1 && trace != 2) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: trace must be 1 or 2");
    if (!(dt >= 0) || !std::isfinite(dt)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: Δt must be finite and non-negative");
    const int N = h->grid.ndim;
    if (h->comm) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: SemiLagrangian runs on a single device (a communicator is attached)");
    for (int d = 0; d < N; ++d) {
        if (h->nloc[d] != h->gn[d] || h->bc[d][0].kind == LSM_BC_NONE || h->bc[d][1].kind == LSM_BC_NONE)
            return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: SemiLagrangian runs on a whole grid, not on a slab");
        if (h->nloc[d] < 2) return lsm_fail(h, LSM_ERR_INVALID, "SemiLagrangian requires at least 2 grid nodes along each dimension");
        if ((h->bc[d][0].kind == LSM_BC_PERIODIC) != (h->bc[d][1].kind == LSM_BC_PERIODIC))
            return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: an axis is periodic on one face only");
    }
    const int ck = term->coeff.kind;
    if (ck != LSM_COEFF_CONST && ck != LSM_COEFF_ROTATION && ck != LSM_COEFF_SEPARABLE && ck != LSM_COEFF_FIELD)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: unknown coefficient kind");
    if (ck == LSM_COEFF_SEPARABLE && term->coeff.time_kind != LSM_TIME_ONE && term->coeff.time_kind != LSM_TIME_COS)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: unknown time factor");
    for (int d = 0; d < N; ++d)
        if ((ck == LSM_COEFF_FIELD && !term->coeff.field[d]) || (ck == LSM_COEFF_SEPARABLE && !term->coeff.sep[d]))
            return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: missing coefficient component");
    const int stage = h->tune.semilag_stage;

    SlArgs a;
    memset(&a, 0, sizeof(a));
    for (int d = 0; d < 3; ++d) {
        a.n[d] = d < N ? h->nloc[d] : 1;
        a.per[d] = d < N && h->bc[d][0].kind == LSM_BC_PERIODIC ? 1 : 0;
        a.lc[d] = h->grid.lc[d];
        a.h[d] = h->h[d];
    }
    a.s1 = h->lay.stride[1]; a.s2 = h->lay.stride[2]; a.origin = h->lay.origin;
    a.dt = dt;
    a.hdt = 0.5 * dt;
    a.trace = trace;
    a.limiter = limiter ? 1 : 0;
    a.f32 = h->dtype == LSM_DTYPE_F32 ? 1 : 0;
    const double tv = trace == 1 ? tc : tc + 0.5 * dt;
    a.vel.kind = ck;
    for (int k = 0; k < 4; ++k) a.vel.v[k] = term->coeff.value[k];
    a.vel.tfac = ck == LSM_COEFF_SEPARABLE && term->coeff.time_kind == LSM_TIME_COS ? cos(M_PI * tv / term->coeff.time_param) : 1.0;
    for (int k = 0; k < 3; ++k) { a.vel.f[k] = (const double*)term->coeff.field[k]; a.vel.sep[k] = term->coeff.sep[k]; }
    a.phi = phi;
    a.out = out;
    // tile of the staged kernel: SL_THREADS·SL_K nodes
    a.tile[0] = N == 1 ? SL_THREADS * SL_K : 32;
    a.tile[1] = N == 1 ? 1 : (N == 2 ? (SL_THREADS / 32) * SL_K : SL_THREADS / 32);
    a.tile[2] = N == 3 ? SL_K : 1;
    const bool use_stage = stage != 0;
    const dim3 grid = sl_grid(N, a, use_stage), sgrid = sl_grid(N, a, true);
    if (grid.y > 65535 || grid.z > 65535 || sgrid.y > 65535 || sgrid.z > 65535)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: grid too large for the launch (65535 workgroups along dimensions 2 and 3)");
    const unsigned long long nwg = (unsigned long long)grid.x * grid.y * grid.z, snwg = (unsigned long long)sgrid.x * sgrid.y * sgrid.z;
    if (nwg >= (1ull << 32) || snwg >= (1ull << 32)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: grid too large (2^32 workgroups)");

    (void)hipSetDevice(h->device);
    hipStream_t st = h->stream;
    if (!h->semilag_ws) h->semilag_ws = new SemilagWorkspace();
    SemilagWorkspace& W = *h->semilag_ws;
    // the counters: one record per workgroup and a reduction behind the launch, only for a caller that asks (or for setting 2)
    auto counters = [&](unsigned long long n) -> int {
        if (!W.stats) LSM_HIP(h, W.stats.alloc(3 * sizeof(unsigned long long)));
        if (!W.h_stats) LSM_HIP(h, W.h_stats.alloc(3 * sizeof(unsigned long long)));
        if (W.rec.cap < n * sizeof(SlRec)) {
            if (W.rec) LSM_HIP(h, hipStreamSynchronize(st));
            LSM_HIP(h, W.rec.alloc(n * sizeof(SlRec)));
        }
        return LSM_OK;
    };
    auto read_counters = [&](unsigned long long n) -> int {
        hipLaunchKernelGGL(semilag_stats_kernel, dim3(1), dim3(SL_THREADS), 0, st, (const SlRec*)W.rec, (unsigned)n, (unsigned long long*)W.stats);
        LSM_HIP(h, hipGetLastError());
        LSM_HIP(h, hipMemcpyAsync(W.h_stats, W.stats, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        LSM_HIP(h, hipStreamSynchronize(st));
        return LSM_OK;
    };

    if (const int rc = lsm_fill_ghosts(h, phi, 7, st); rc != LSM_OK) return rc;
    if (stage == 2) {
        // every workgroup must stage: count first, write nothing
        if (const int rc = counters(snwg); rc != LSM_OK) return rc;
        a.mode = 2;
        a.rec = W.rec;
        sl_launch_n(N, a, order, true, st);
        LSM_HIP(h, hipGetLastError());
        if (const int rc = read_counters(snwg); rc != LSM_OK) return rc;
        if (W.h_stats.p[1] != 0) {
            if (stats) { stats[0] = (int64_t)W.h_stats.p[0]; stats[1] = (int64_t)W.h_stats.p[1]; stats[2] = 0; }
            return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_semilag: LSM_SEMILAG_STAGE=2 and " + std::to_string(W.h_stats.p[1]) +
                                                    " workgroups' departure boxes do not fit the staged tile; out is unchanged");
        }
    }
    a.mode = 1;
    a.rec = nullptr;
    if (stats) {
        if (const int rc = counters(nwg); rc != LSM_OK) return rc;
        a.rec = W.rec;
    }
    sl_launch_n(N, a, order, use_stage, st);
    LSM_HIP(h, hipGetLastError());
    if (stats) {
        if (const int rc = read_counters(nwg); rc != LSM_OK) return rc;
        stats[0] = (int64_t)W.h_stats.p[0];
        stats[1] = (int64_t)W.h_stats.p[1];
        double m;
        memcpy(&m, &W.h_stats.p[2], sizeof(m));
        stats[2] = m < 9.0e18 ? (int64_t)std::ceil(m) : INT64_MAX;
    }
    return LSM_OK;
}
