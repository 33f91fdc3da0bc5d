// lsm_elliptic.hip — elliptic_solve: −∇·(a∇u) + c·u = f on the box of a dense 2-D / 3-D grid with an ersatz material outside the
// level set, solved on the device by conjugate gradients preconditioned with one geometric multigrid V-cycle (or with the
// diagonal).  DESIGN.md §7.17; include/lsm.h ("elliptic_solve") states the discretisation, tests/_elliptic_ref.py restates it.
// Built with -ffp-contract=off: the cell array, A x and the energy density round as numpy does.
//
// Storage.  Solver vectors are fp64 over the compact node index id = i0 + n0·(i1 + n1·i2); the cell array of a level has n−1
// entries per axis, axis 0 fastest.  The operator is never stored: a node loads the 2^N cells around it (zero where there is
// none; adding +0 is exact, so the sums equal those over the existing cells) and forms its 2N edge coefficients from them —
// 8 bytes per node from HBM instead of the 8·N of stored edge arrays.  The diagonal is stored (the smoother and the Jacobi
// preconditioner divide by it).  u is read once (the guess and the Dirichlet values) and written once (the free nodes).
//
// One PCG iteration:
//   [z = M r, ρ' = r·z, β = ρ'/ρ]   the V-cycle, whose last sweep carries the dot product — or, for M = D⁻¹, part of K2
//   K1  p' = z + β p (p double-buffered: neighbours read the old one),  q = A p',  σ = p'·q   → α = ρ/σ
//   K2  x += α p',  r −= α q,  r·r → converged?  (Jacobi: z = r/D, ρ' = r·z as well)
// Reductions by wave.h's block_reduce_ordered: one partial per workgroup, the last workgroup to draw a ticket sums them in workgroup order and
// updates the scalars; every kernel returns at once when the device status is set, the host enqueues iterations in chunks and
// reads the status once per chunk.
//
// The V-cycle (from zero, for A x = r on the free nodes; ω = 0.8):
//   per level but the coarsest:  x = ω r/D;  x ← x + ω (r − A x)/D;  r_c = Pᵀ(r − A x)/2^k (the fine residual written once into the
//   level's free smoother buffer, then gathered: the one-kernel form, in which a coarse node evaluates the residuals of the ≤ 3^N
//   fine nodes it gathers from, is kept as -DLSM_EL_SPLIT_RESTRICT=0 and lost, 219 against 168 ms per 256³ solve: DESIGN.md §7.17);
//   …coarser levels…;  x += P x_c (one kernel, in place);  two more sweeps.
//   The coarsest level (≤ 5 nodes per axis, so ≤ 125 nodes): 16 sweeps from zero in ONE single-workgroup kernel, x in LDS.
//   Fixed nodes: residuals and corrections are zero there; a coarse node is fixed iff fine node 2J is.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "el_cell.h"
#include "lsm_handle.h"
#include "wave.h"

namespace lsm {

// the measured choice; a variant library for tools/elliptic_bench.py is built with -DLSM_EL_SPLIT_RESTRICT=0 / 1
#ifndef LSM_EL_SPLIT_RESTRICT
#define LSM_EL_SPLIT_RESTRICT 1
#endif
static const int EL_THREADS = 256;
static const int EL_MAXB = 2048;
static const int EL_NCOARSE = 16;
static const double EL_OMEGA = 0.8;
enum { EL_RUN = 0, EL_CONVERGED = 1, EL_MAXITER = 2, EL_BREAK_INPUT = -1, EL_BREAK_SIGMA = -2, EL_BREAK_RHO = -3 };
enum { EL_BAD_PHI = 0, EL_BAD_A = 1, EL_BAD_C = 2, EL_NFIXED = 3, EL_CPOS = 4, EL_NSTAT = 8 };

struct ElState {
    double rho, alpha, beta, bb, rr, rtol2, out;
    int status, iters, max_iters, first;
    unsigned long long nonfinite;
    unsigned ticket[4];
};

struct ElLevel {
    int n[3];
    int nn;
    double h[3], ih2[3];
    const double* a;              // cells, n−1 per axis
    const double* cn;             // c per node, or NULL: cc everywhere
    double cc;
    const unsigned char* fixed;   // one byte per node, or NULL: no fixed node
    const double* D;              // the diagonal
};

// where the field of the handle lives (padded layout), for the kernels that read or write one
struct ElField { long long s1, s2, origin; int f32; };

template <int N>
__device__ __forceinline__ void el_coords(const ElLevel& L, int id, int I[3]) {
    I[0] = id % L.n[0];
    const int r = id / L.n[0];
    I[1] = N > 2 ? r % L.n[1] : r;
    I[2] = N > 2 ? r / L.n[1] : 0;
}
__device__ __forceinline__ long long el_padded(const ElField& F, const int I[3]) { return F.origin + I[0] + I[1] * F.s1 + I[2] * F.s2; }
__device__ __forceinline__ bool el_fixed(const ElLevel& L, int id) { return L.fixed && L.fixed[id]; }

// the 2^N cells around node I: bit d of m set: cell index I_d along d, clear: I_d − 1; zero where there is no cell
template <int N>
__device__ __forceinline__ void el_cells_around(const ElLevel& L, const int I[3], double v[1 << N]) {
    const int c0 = L.n[0] - 1, c1 = L.n[1] - 1;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {
        int C[3] = {0, 0, 0};
        bool in = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            C[d] = I[d] - 1 + ((m >> d) & 1);
            in = in && C[d] >= 0 && C[d] < L.n[d] - 1;
        }
        v[m] = in ? L.a[C[0] + c0 * (C[1] + (N > 2 ? c1 * C[2] : 0))] : 0.0;
    }
}
// S of the edge along d on side s (0: towards I − e_d, 1: towards I + e_d): the cells with bit d = s, ascending
template <int N>
__device__ __forceinline__ double el_edge_sum(const double v[1 << N], int d, int s) {
    double S = 0.0;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m)
        if (((m >> d) & 1) == s) S = S + v[m];
    return S;
}
template <int N>
__device__ __forceinline__ double el_mass(const ElLevel& L, const int I[3]) {
    double m = 1.0;
#pragma unroll
    for (int d = 0; d < N; ++d)
        if (I[d] == 0 || I[d] == L.n[d] - 1) m = m * 0.5;
    return m;
}
template <int N>
__device__ __forceinline__ double el_cm(const ElLevel& L, int id, const int I[3]) { return (L.cn ? L.cn[id] : L.cc) * el_mass<N>(L, I); }

// (A x)_I in the stated order; xat(id) gives x at a neighbour
template <int N, class X>
__device__ __forceinline__ double el_apply(const ElLevel& L, int id, const int I[3], double xi, X xat) {
    double v[1 << N];
    el_cells_around<N>(L, I, v);
    const int cs[3] = {1, L.n[0], L.n[0] * L.n[1]};
    const double half = N == 2 ? 0.5 : 0.25;
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        if (I[d] > 0) acc = acc + ((el_edge_sum<N>(v, d, 0) * half) * L.ih2[d]) * (xi - xat(id - cs[d]));
        if (I[d] < L.n[d] - 1) acc = acc + ((el_edge_sum<N>(v, d, 1) * half) * L.ih2[d]) * (xi - xat(id + cs[d]));
    }
    return acc + el_cm<N>(L, id, I) * xi;
}
// the eliminated operator at a free node: fixed neighbours count as zero
template <int N>
__device__ __forceinline__ double el_apply_free(const ElLevel& L, int id, const int I[3], const double* __restrict__ x) {
    return el_apply<N>(L, id, I, x[id], [&](int q) { return el_fixed(L, q) ? 0.0 : x[q]; });
}

__device__ __forceinline__ bool el_finite(double x) { return x - x == 0.0; }

#define EL_LOOP(id, nn) for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < (nn); id += gridDim.x * blockDim.x)

// ---- setup of level 0: the cell array from ϕ (or the caller's, checked), c checked, fixed nodes counted.  One thread per node;
// a node that is the lowest corner of a cell writes that cell.
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_setup_kernel(ElLevel L, ElField F, const void* __restrict__ phi, double level, double a_in, double a_out,
                                                              double hmin, const double* __restrict__ a_given, double* __restrict__ a, unsigned long long* st) {
    unsigned cnt[5] = {0, 0, 0, 0, 0};      // per thread, added once per wave: one atomic per node on one word serialises the launch
    EL_LOOP(id, L.nn) {
        int I[3];
        el_coords<N>(L, id, I);
        if (phi && !el_finite(ld_val(phi, el_padded(F, I), F.f32))) ++cnt[EL_BAD_PHI];
        const double c = L.cn ? L.cn[id] : L.cc;
        if (!(c >= 0.0) || !el_finite(c)) ++cnt[EL_BAD_C];
        else if (c > 0.0) ++cnt[EL_CPOS];
        if (el_fixed(L, id)) ++cnt[EL_NFIXED];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && I[d] < L.n[d] - 1;
        if (!corner) continue;
        const int ci = I[0] + (L.n[0] - 1) * (I[1] + (N > 2 ? (L.n[1] - 1) * I[2] : 0));
        double av;
        if (a_given) {
            av = a_given[ci];
            if (!(av > 0.0) || !el_finite(av)) ++cnt[EL_BAD_A];
        } else {
            av = el_cell_from_phi<N>(phi, el_padded(F, I), F.s1, F.s2, F.f32, level, a_in, a_out, hmin);
        }
        a[ci] = av;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned v = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&st[k], (unsigned long long)v);
    }
}

// ---- a coarse level from the fine one: cells averaged, c and the fixed mask injected.  co: the axes that coarsen
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_coarsen_kernel(ElLevel Lf, ElLevel Lc, int co0, int co1, int co2, double* __restrict__ ac,
                                                                double* __restrict__ cnc, unsigned char* __restrict__ fixc) {
    const int co[3] = {co0, co1, co2};
    const int k = co0 + co1 + co2;
    const double scale = k == 1 ? 0.5 : k == 2 ? 0.25 : 0.125;
    EL_LOOP(id, Lc.nn) {
        int J[3];
        el_coords<N>(Lc, id, J);
        const int fid = (co[0] ? 2 * J[0] : J[0]) + Lf.n[0] * ((co[1] ? 2 * J[1] : J[1]) + (N > 2 ? Lf.n[1] * (co[2] ? 2 * J[2] : J[2]) : 0));
        if (cnc) cnc[id] = Lf.cn[fid];
        if (fixc) fixc[id] = Lf.fixed[fid];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && J[d] < Lc.n[d] - 1;
        if (!corner) continue;
        double s = 0.0;
        bool first = true;
#pragma unroll
        for (int m = 0; m < (1 << N); ++m) {    // the fine cells {2J, 2J+1} per coarsened axis, ascending
            int C[3] = {0, 0, 0};
            bool use = true;
#pragma unroll
            for (int d = 0; d < N; ++d) {
                const int b = (m >> d) & 1;
                if (!co[d] && b) use = false;
                C[d] = co[d] ? 2 * J[d] + b : J[d];
            }
            if (!use) continue;
            const double v = Lf.a[C[0] + (Lf.n[0] - 1) * (C[1] + (N > 2 ? (Lf.n[1] - 1) * C[2] : 0))];
            s = first ? v : s + v;
            first = false;
        }
        ac[J[0] + (Lc.n[0] - 1) * (J[1] + (N > 2 ? (Lc.n[1] - 1) * J[2] : 0))] = s * scale;
    }
}

// ---- the diagonal of a level
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_diag_kernel(ElLevel L, double* __restrict__ D) {
    const double half = N == 2 ? 0.5 : 0.25;
    EL_LOOP(id, L.nn) {
        int I[3];
        el_coords<N>(L, id, I);
        double v[1 << N];
        el_cells_around<N>(L, I, v);
        double acc = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            if (I[d] > 0) acc = acc + (el_edge_sum<N>(v, d, 0) * half) * L.ih2[d];
            if (I[d] < L.n[d] - 1) acc = acc + (el_edge_sum<N>(v, d, 1) * half) * L.ih2[d];
        }
        D[id] = acc + el_cm<N>(L, id, I);
    }
}

// ---- y = A x on all nodes, no elimination (lsm_elliptic_apply)
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_apply_kernel(ElLevel L, const double* __restrict__ x, double* __restrict__ y) {
    EL_LOOP(id, L.nn) {
        int I[3];
        el_coords<N>(L, id, I);
        y[id] = el_apply<N>(L, id, I, x[id], [&](int q) { return x[q]; });
    }
}

// ---- the energy density e_I = Σ_d (Σ_± k̄·(g·g), g = (u_J − u_I)/h_d)/(existing edges along d at I), into a field of the handle
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_energy_kernel(ElLevel L, ElField F, const void* __restrict__ u, void* __restrict__ e_out) {
    EL_LOOP(id, L.nn) {
        int I[3];
        el_coords<N>(L, id, I);
        double v[1 << N];
        el_cells_around<N>(L, I, v);
        const long long at = el_padded(F, I);
        const long long fs[3] = {1, F.s1, F.s2};
        const double ui = ld_val(u, at, F.f32);
        double e = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            // the cells an edge along d has: one per pair of sides of the other axes that exist
            double ncell = 1.0;
#pragma unroll
            for (int o = 0; o < N; ++o)
                if (o != d && I[o] > 0 && I[o] < L.n[o] - 1) ncell = ncell * 2.0;
            double s = 0.0, cnt = 0.0;
            if (I[d] > 0) {
                const double g = (ld_val(u, at - fs[d], F.f32) - ui) / L.h[d];
                s = s + (el_edge_sum<N>(v, d, 0) / ncell) * (g * g);
                cnt = cnt + 1.0;
            }
            if (I[d] < L.n[d] - 1) {
                const double g = (ld_val(u, at + fs[d], F.f32) - ui) / L.h[d];
                s = s + (el_edge_sum<N>(v, d, 1) / ncell) * (g * g);
                cnt = cnt + 1.0;
            }
            e = e + s / cnt;
        }
        st_val(e_out, at, F.f32, e);
    }
}

// ---- Πh·Σ m f u is finished on the host: this reduces Σ (m·f)·u
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_compliance_kernel(ElLevel L, ElField F, const double* __restrict__ f, const void* __restrict__ u,
                                                                   double* partial, ElState* st) {
    double red[1] = {0.0};
    EL_LOOP(id, L.nn) {
        int I[3];
        el_coords<N>(L, id, I);
        red[0] += (el_mass<N>(L, I) * f[id]) * ld_val(u, el_padded(F, I), F.f32);
    }
    if (!block_reduce_ordered<1, EL_THREADS>(red, partial, &st->ticket[3]) || threadIdx.x != 0) return;
    st->out = red[0];
}

// ---- PCG
struct ElVec {
    double *x, *r, *q, *p[2], *z;   // z: where the preconditioner leaves M r
    double* partial;
    ElState* st;
};

// x₀ = u (the guess and the Dirichlet values), b = m·f, r₀ = b − A x₀ on the free nodes, 0 on the fixed ones; ‖b_free‖², ‖r₀‖²;
// jac: z = r/D and ρ = r·z as well
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_init_kernel(ElLevel L, ElField F, ElVec V, const double* __restrict__ f, const void* __restrict__ u, int jac) {
    double red[4] = {0.0, 0.0, 0.0, 0.0};     // ‖b_free‖², ‖r₀‖², r·z, non-finite entries (a count below 2^53: exact)
    EL_LOOP(id, L.nn) {
        int I[3];
        el_coords<N>(L, id, I);
        const long long at = el_padded(F, I);
        const long long fs[3] = {1, F.s1, F.s2};
        const int cs[3] = {1, L.n[0], L.n[0] * L.n[1]};
        const double ui = ld_val(u, at, F.f32), fi = f[id];
        if (!el_finite(ui) || !el_finite(fi)) red[3] += 1.0;
        double r = 0.0, z = 0.0;
        if (!el_fixed(L, id)) {
            const double b = el_mass<N>(L, I) * fi;
            const double ax = el_apply<N>(L, id, I, ui, [&](int q) {
                const int dq = q - id;
                const long long o = dq == -cs[0] ? -fs[0] : dq == cs[0] ? fs[0] : dq == -cs[1] ? -fs[1] : dq == cs[1] ? fs[1] : dq < 0 ? -fs[2] : fs[2];
                return ld_val(u, at + o, F.f32);
            });
            r = b - ax;
            red[0] += b * b;
            red[1] += r * r;
            if (jac) {
                z = r / L.D[id];
                red[2] += r * z;
            }
        }
        V.x[id] = ui;
        V.r[id] = r;
        V.p[0][id] = 0.0;
        if (jac) V.z[id] = z;
    }
    if (!block_reduce_ordered<4, EL_THREADS>(red, V.partial, &V.st->ticket[0]) || threadIdx.x != 0) return;
    ElState& S = *V.st;
    S.bb = red[0] > 0.0 ? red[0] : red[1];      // f ≡ 0 on the free nodes: the norm of the eliminated right-hand side
    S.rr = red[1];
    S.rho = red[2];
    S.alpha = 0.0; S.beta = 0.0;
    S.iters = 0;
    S.first = 1;
    S.nonfinite = (unsigned long long)red[3];
    if (red[3] > 0.0 || !el_finite(red[0]) || !el_finite(red[1])) S.status = EL_BREAK_INPUT;
    else if (red[1] <= S.rtol2 * S.bb) S.status = EL_CONVERGED;
    else if (jac && !(red[2] > 0.0)) S.status = EL_BREAK_RHO;
    else S.status = EL_RUN;
    if (jac) S.first = 0;
}

// K1: p' = z + β p, q = A p' (eliminated), σ = p'·q, α = ρ/σ
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_k1_kernel(ElLevel L, ElVec V, int par) {
    if (V.st->status != EL_RUN) return;
    const double beta = V.st->beta;
    const double* __restrict__ z = V.z;
    const double* __restrict__ po = V.p[par];
    double* __restrict__ pn = V.p[par ^ 1];
    double red[1] = {0.0};
    EL_LOOP(id, L.nn) {
        double pp = 0.0, q = 0.0;
        if (!el_fixed(L, id)) {
            int I[3];
            el_coords<N>(L, id, I);
            pp = z[id] + beta * po[id];
            q = el_apply<N>(L, id, I, pp, [&](int j) { return el_fixed(L, j) ? 0.0 : z[j] + beta * po[j]; });
            red[0] += pp * q;
        }
        pn[id] = pp;
        V.q[id] = q;
    }
    if (!block_reduce_ordered<1, EL_THREADS>(red, V.partial, &V.st->ticket[1]) || threadIdx.x != 0) return;
    ElState& S = *V.st;
    const double alpha = S.rho / red[0];
    if (!(red[0] > 0.0) || !el_finite(alpha)) { S.status = EL_BREAK_SIGMA; return; }
    S.alpha = alpha;
}

// K2: x += α p', r −= α q, r·r → converged?; JAC: z = r/D, ρ' = r·z, β = ρ'/ρ
template <int JAC>
__global__ void __launch_bounds__(EL_THREADS) el_k2_kernel(ElLevel L, ElVec V, int par) {
    if (V.st->status != EL_RUN) return;
    const double alpha = V.st->alpha;
    const double* __restrict__ p = V.p[par ^ 1];
    double red[2] = {0.0, 0.0};
    EL_LOOP(id, L.nn) {
        V.x[id] = V.x[id] + alpha * p[id];
        const double r = V.r[id] - alpha * V.q[id];
        V.r[id] = r;
        red[0] += r * r;
        if (JAC) {
            const double z = r / L.D[id];      // r is zero on the fixed nodes
            V.z[id] = z;
            red[1] += r * z;
        }
    }
    if (!block_reduce_ordered<2, EL_THREADS>(red, V.partial, &V.st->ticket[2]) || threadIdx.x != 0) return;
    ElState& S = *V.st;
    S.iters += 1;
    S.rr = red[0];
    if (red[0] <= S.rtol2 * S.bb) { S.status = EL_CONVERGED; return; }
    if (!el_finite(red[0])) { S.status = EL_BREAK_RHO; return; }
    if (JAC) {
        if (!(red[1] > 0.0) || !el_finite(red[1])) { S.status = EL_BREAK_RHO; return; }
        S.beta = red[1] / S.rho;
        S.rho = red[1];
    }
    if (S.iters >= S.max_iters) S.status = EL_MAXITER;
}

// the scalars after z = M r of the V-cycle: ρ' = r·z, β = ρ'/ρ (0 the first time)
__device__ __forceinline__ void el_rho_update(ElState& S, double rz) {
    if (!(rz > 0.0) || !el_finite(rz)) { S.status = EL_BREAK_RHO; return; }
    S.beta = S.first ? 0.0 : rz / S.rho;
    S.rho = rz;
    S.first = 0;
}

// ---- the V-cycle's kernels (any level)
// first sweep from zero: x = ω r/D
__global__ void __launch_bounds__(EL_THREADS) el_smooth0_kernel(ElLevel L, const double* __restrict__ r, double* __restrict__ x, const ElState* st) {
    if (st->status != EL_RUN) return;
    EL_LOOP(id, L.nn) x[id] = el_fixed(L, id) ? 0.0 : (EL_OMEGA * r[id]) / L.D[id];
}
// xn = x + ω (r − A x)/D; DOT (the cycle's last sweep on level 0): r·xn and the scalars
template <int N, int DOT>
__global__ void __launch_bounds__(EL_THREADS) el_smooth_kernel(ElLevel L, const double* __restrict__ r, const double* __restrict__ x, double* __restrict__ xn,
                                                               double* partial, ElState* st) {
    if (st->status != EL_RUN) return;
    double red[1] = {0.0};
    EL_LOOP(id, L.nn) {
        double v = 0.0;
        if (!el_fixed(L, id)) {
            int I[3];
            el_coords<N>(L, id, I);
            v = x[id] + (EL_OMEGA * (r[id] - el_apply_free<N>(L, id, I, x))) / L.D[id];
            if (DOT) red[0] += r[id] * v;
        }
        xn[id] = v;
    }
    if (DOT) {
        if (!block_reduce_ordered<1, EL_THREADS>(red, partial, &st->ticket[3]) || threadIdx.x != 0) return;
        el_rho_update(*st, red[0]);
    }
}
// the one-pass form (LSM_EL_SPLIT_RESTRICT=0; measured and lost).  r_c = Pᵀ (r − A x)_free / 2^k: a coarse node gathers the residuals of the fine nodes 2J + o, o ∈ {−1, 0, 1} per coarsened axis
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_restrict_kernel(ElLevel Lf, ElLevel Lc, int co0, int co1, int co2, const double* __restrict__ r,
                                                                 const double* __restrict__ x, double* __restrict__ rc, const ElState* st) {
    if (st->status != EL_RUN) return;
    const int co[3] = {co0, co1, co2};
    const int k = co0 + co1 + co2;
    const double scale = k == 1 ? 0.5 : k == 2 ? 0.25 : 0.125;
    EL_LOOP(id, Lc.nn) {
        double acc = 0.0;
        if (!el_fixed(Lc, id)) {
            int J[3];
            el_coords<N>(Lc, id, J);
            for (int m = 0; m < (N == 2 ? 9 : 27); ++m) {
                const int o[3] = {m % 3 - 1, (m / 3) % 3 - 1, N > 2 ? m / 9 - 1 : 0};
                int I[3] = {0, 0, 0};
                double w = 1.0;
                bool use = true;
#pragma unroll
                for (int d = 0; d < N; ++d) {
                    if (!co[d]) {
                        if (o[d] != 0) use = false;
                        I[d] = J[d];
                        continue;
                    }
                    I[d] = 2 * J[d] + o[d];
                    if (I[d] < 0 || I[d] >= Lf.n[d]) use = false;
                    if (o[d] == -1 || (o[d] == 1 && J[d] + 1 < Lc.n[d])) w = w * 0.5;     // the unpaired last fine node gives all it has
                }
                if (!use) continue;
                const int fid = I[0] + Lf.n[0] * (I[1] + (N > 2 ? Lf.n[1] * I[2] : 0));
                if (el_fixed(Lf, fid)) continue;
                acc += w * (r[fid] - el_apply_free<N>(Lf, fid, I, x));
            }
        }
        rc[id] = acc * scale;
    }
}
// the two-pass form (LSM_EL_SPLIT_RESTRICT=1, the default): the fine residual written once (into the level's free smoother buffer), then gathered
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_resid_kernel(ElLevel L, const double* __restrict__ r, const double* __restrict__ x, double* __restrict__ res,
                                                              const ElState* st) {
    if (st->status != EL_RUN) return;
    EL_LOOP(id, L.nn) {
        double v = 0.0;
        if (!el_fixed(L, id)) {
            int I[3];
            el_coords<N>(L, id, I);
            v = r[id] - el_apply_free<N>(L, id, I, x);
        }
        res[id] = v;
    }
}
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_gather_kernel(ElLevel Lf, ElLevel Lc, int co0, int co1, int co2, const double* __restrict__ res,
                                                               double* __restrict__ rc, const ElState* st) {
    if (st->status != EL_RUN) return;
    const int co[3] = {co0, co1, co2};
    const int k = co0 + co1 + co2;
    const double scale = k == 1 ? 0.5 : k == 2 ? 0.25 : 0.125;
    EL_LOOP(id, Lc.nn) {
        double acc = 0.0;
        if (!el_fixed(Lc, id)) {
            int J[3];
            el_coords<N>(Lc, id, J);
            for (int m = 0; m < (N == 2 ? 9 : 27); ++m) {
                const int o[3] = {m % 3 - 1, (m / 3) % 3 - 1, N > 2 ? m / 9 - 1 : 0};
                int I[3] = {0, 0, 0};
                double w = 1.0;
                bool use = true;
#pragma unroll
                for (int d = 0; d < N; ++d) {
                    if (!co[d]) {
                        if (o[d] != 0) use = false;
                        I[d] = J[d];
                        continue;
                    }
                    I[d] = 2 * J[d] + o[d];
                    if (I[d] < 0 || I[d] >= Lf.n[d]) use = false;
                    if (o[d] == -1 || (o[d] == 1 && J[d] + 1 < Lc.n[d])) w = w * 0.5;
                }
                if (use) acc += w * res[I[0] + Lf.n[0] * (I[1] + (N > 2 ? Lf.n[1] * I[2] : 0))];     // zero on fixed fine nodes
            }
        }
        rc[id] = acc * scale;
    }
}
// x += P x_c on the free fine nodes
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_prolong_kernel(ElLevel Lf, ElLevel Lc, int co0, int co1, int co2, const double* __restrict__ xc,
                                                                double* __restrict__ x, const ElState* st) {
    if (st->status != EL_RUN) return;
    const int co[3] = {co0, co1, co2};
    EL_LOOP(id, Lf.nn) {
        if (el_fixed(Lf, id)) continue;
        int I[3];
        el_coords<N>(Lf, id, I);
        int J0[3] = {0, 0, 0}, two[3] = {0, 0, 0};
#pragma unroll
        for (int d = 0; d < N; ++d) {
            J0[d] = co[d] ? I[d] >> 1 : I[d];
            two[d] = co[d] && (I[d] & 1) && J0[d] + 1 < Lc.n[d];
        }
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < (1 << N); ++m) {
            double w = 1.0;
            bool use = true;
            int J[3] = {0, 0, 0};
#pragma unroll
            for (int d = 0; d < N; ++d) {
                const int b = (m >> d) & 1;
                if (b && !two[d]) use = false;
                if (two[d]) w = w * 0.5;
                J[d] = J0[d] + b;
            }
            if (use) acc += w * xc[J[0] + Lc.n[0] * (J[1] + (N > 2 ? Lc.n[1] * J[2] : 0))];
        }
        x[id] = x[id] + acc;
    }
}
// the coarsest level (≤ 128 nodes): EL_NCOARSE sweeps from zero in one workgroup, x in LDS, double-buffered
template <int N, int DOT>
__global__ void __launch_bounds__(128) el_coarsest_kernel(ElLevel L, const double* __restrict__ r, double* __restrict__ x, ElState* st) {
    __shared__ double xs[2][128];
    __shared__ double red[2];
    if (st->status != EL_RUN) return;
    const int id = threadIdx.x;
    const bool on = id < L.nn && !el_fixed(L, id);
    int I[3] = {0, 0, 0};
    if (id < L.nn) el_coords<N>(L, id, I);
    const double ri = on ? r[id] : 0.0, Di = on ? L.D[id] : 1.0;
    double v = on ? (EL_OMEGA * ri) / Di : 0.0;
    int cur = 0;
    for (int s = 1; s < EL_NCOARSE; ++s) {
        xs[cur][id] = v;
        __syncthreads();
        if (on) {
            const double* xb = xs[cur];
            v = v + (EL_OMEGA * (ri - el_apply<N>(L, id, I, v, [&](int q) { return xb[q]; }))) / Di;     // fixed nodes hold zero
        }
        cur ^= 1;
    }
    if (id < L.nn) x[id] = v;
    if (DOT) {
        const double s = wave_sum(ri * v);
        if ((id & 63) == 0) red[id >> 6] = s;
        __syncthreads();
        if (id == 0) el_rho_update(*st, red[0] + red[1]);
    }
}

// ---- x → u on the free nodes (rounded to the storage type); the fixed nodes and the ghosts are left as they are
template <int N>
__global__ void __launch_bounds__(EL_THREADS) el_store_kernel(ElLevel L, ElField F, const double* __restrict__ x, void* __restrict__ u) {
    EL_LOOP(id, L.nn) {
        if (el_fixed(L, id)) continue;
        int I[3];
        el_coords<N>(L, id, I);
        st_val(u, el_padded(F, I), F.f32, x[id]);
    }
}

// ---- host side
struct EllipticObject {
    int N = 0, precond = 0, last_iters = 0;
    int co[32][3];                       // co[l]: the axes that coarsen from level l to l+1
    std::vector<ElLevel> lev;
    std::vector<double*> rhs, xa, xb;    // per level ≥ 1: right-hand side and the two smoother buffers; level 0: xa, xb only
    ElVec V;
    ElField F;
    long long nfree = 0, nfixed = 0;
    DevBuf<double> buf, partial;
    DevBuf<unsigned char> fx;
    DevBuf<ElState> st;
    DevBuf<unsigned long long> cnt;
    PinnedBuf<ElState> h_st;
};

static unsigned el_blocks(long long n) { return (unsigned)std::min<long long>((n + EL_THREADS - 1) / EL_THREADS, EL_MAXB); }

#define EL_LAUNCH(N, kernel, grid, block, stream, ...)                                              \
    do {                                                                                            \
        if ((N) == 2) hipLaunchKernelGGL(kernel<2>, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<3>, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);        \
    } while (0)
#define EL_LAUNCH2(N, kernel, flag, grid, block, stream, ...)                                               \
    do {                                                                                                    \
        if ((N) == 2) hipLaunchKernelGGL((kernel<2, flag>), dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
        else hipLaunchKernelGGL((kernel<3, flag>), dim3(grid), dim3(block), 0, stream, __VA_ARGS__);        \
    } while (0)

// z = M r for M = one V-cycle; the last kernel leaves ρ and β
static void el_vcycle(EllipticObject& o, hipStream_t s) {
    const int N = o.N, nl = (int)o.lev.size();
    ElState* st = o.st;
    for (int l = 0; l + 1 < nl; ++l) {
        const ElLevel& L = o.lev[l];
        const double* r = l == 0 ? o.V.r : o.rhs[l];
        const unsigned nb = el_blocks(L.nn);
        hipLaunchKernelGGL(el_smooth0_kernel, dim3(nb), dim3(EL_THREADS), 0, s, L, r, o.xa[l], (const ElState*)st);
        EL_LAUNCH2(N, el_smooth_kernel, 0, nb, EL_THREADS, s, L, r, (const double*)o.xa[l], o.xb[l], o.partial.p, st);
#if LSM_EL_SPLIT_RESTRICT
        EL_LAUNCH(N, el_resid_kernel, nb, EL_THREADS, s, L, r, (const double*)o.xb[l], o.xa[l], (const ElState*)st);      // xa is free until the post-smoothing
        EL_LAUNCH(N, el_gather_kernel, el_blocks(o.lev[l + 1].nn), EL_THREADS, s, L, o.lev[l + 1], o.co[l][0], o.co[l][1], o.co[l][2],
                  (const double*)o.xa[l], o.rhs[l + 1], (const ElState*)st);
#else
        EL_LAUNCH(N, el_restrict_kernel, el_blocks(o.lev[l + 1].nn), EL_THREADS, s, L, o.lev[l + 1], o.co[l][0], o.co[l][1], o.co[l][2], r,
                  (const double*)o.xb[l], o.rhs[l + 1], (const ElState*)st);
#endif
    }
    {
        const int l = nl - 1;
        const double* r = l == 0 ? o.V.r : o.rhs[l];
        if (l == 0) EL_LAUNCH2(N, el_coarsest_kernel, 1, 1, 128, s, o.lev[l], r, o.xb[l], st);
        else EL_LAUNCH2(N, el_coarsest_kernel, 0, 1, 128, s, o.lev[l], r, o.xb[l], st);
    }
    for (int l = nl - 2; l >= 0; --l) {
        const ElLevel& L = o.lev[l];
        const double* r = l == 0 ? o.V.r : o.rhs[l];
        const unsigned nb = el_blocks(L.nn);
        EL_LAUNCH(N, el_prolong_kernel, nb, EL_THREADS, s, L, o.lev[l + 1], o.co[l][0], o.co[l][1], o.co[l][2], (const double*)o.xb[l + 1], o.xb[l],
                  (const ElState*)st);
        EL_LAUNCH2(N, el_smooth_kernel, 0, nb, EL_THREADS, s, L, r, (const double*)o.xb[l], o.xa[l], o.partial.p, st);
        if (l == 0) EL_LAUNCH2(N, el_smooth_kernel, 1, nb, EL_THREADS, s, L, r, (const double*)o.xa[l], o.xb[l], o.partial.p, st);
        else EL_LAUNCH2(N, el_smooth_kernel, 0, nb, EL_THREADS, s, L, r, (const double*)o.xa[l], o.xb[l], o.partial.p, st);
    }
}

}  // namespace lsm

using namespace lsm;

struct LsmElliptic { LsmHandle* h; EllipticObject* o; };

#define EL_HIP(h, call)                                                                                       \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) return lsm_fail(h, LSM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

static int el_create(LsmHandle* h, EllipticObject& o, const void* phi, double level, double a_in, double a_out, const double* a_cells, double c_const,
                     const double* c_nodes, const unsigned char* fixed, int64_t stats[4]) {
    const int N = h->grid.ndim;
    o.N = N;
    o.F = ElField{h->lay.stride[1], N > 2 ? h->lay.stride[2] : 0, h->lay.origin, h->dtype == LSM_DTYPE_F32 ? 1 : 0};
    // the hierarchy's shapes: axis d coarsens while n_d > 5, to (n_d+1)/2 nodes; it ends when no axis coarsens
    std::vector<ElLevel> lev;
    ElLevel L;
    memset(&L, 0, sizeof(L));
    long long nn = 1;
    double hmin = INFINITY;
    for (int d = 0; d < 3; ++d) {
        L.n[d] = d < N ? h->nloc[d] : 1;
        L.h[d] = d < N ? h->h[d] : 1.0;
        L.ih2[d] = 1.0 / (L.h[d] * L.h[d]);
        nn *= L.n[d];
        if (d < N) hmin = std::min(hmin, L.h[d]);
    }
    if (nn >= (1LL << 31) / 4) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: the grid is too large (2^29 nodes at most)");
    L.nn = (int)nn;
    L.cc = c_const;
    lev.push_back(L);
    for (;;) {
        const ElLevel& f = lev.back();
        ElLevel c = f;
        bool any = false;
        const int l = (int)lev.size() - 1;
        c.nn = 1;
        for (int d = 0; d < 3; ++d) {
            o.co[l][d] = d < N && f.n[d] > 5;
            if (o.co[l][d]) {
                any = true;
                c.n[d] = (f.n[d] + 1) / 2;
                c.h[d] = f.h[d] * 2.0;
                c.ih2[d] = 1.0 / (c.h[d] * c.h[d]);
            }
            c.nn *= c.n[d];
        }
        if (!any || lev.size() >= 31) break;
        lev.push_back(c);
    }
    const int nl = (int)lev.size();
    if (lev[nl - 1].nn > 128) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: the coarsest level has more than 128 nodes");
    // one allocation of doubles: per level cells, D, [c], xa, xb, [rhs]; level 0: x r q p0 p1 as well
    auto ncell = [&](const ElLevel& q) { long long m = 1; for (int d = 0; d < N; ++d) m *= q.n[d] - 1; return m; };
    size_t nd = 0, nb = 0;
    for (int l = 0; l < nl; ++l) {
        nd += (size_t)ncell(lev[l]) + (size_t)lev[l].nn * (size_t)(3 + (c_nodes ? 1 : 0) + (l ? 1 : 5));
        nb += (size_t)lev[l].nn;
    }
    EL_HIP(h, o.buf.alloc(nd * sizeof(double)));
    if (fixed) EL_HIP(h, o.fx.alloc(nb));
    EL_HIP(h, o.partial.alloc(4 * EL_MAXB * sizeof(double)));
    EL_HIP(h, o.st.alloc(sizeof(ElState)));
    EL_HIP(h, o.cnt.alloc(EL_NSTAT * sizeof(unsigned long long)));
    EL_HIP(h, o.h_st.alloc(sizeof(ElState)));
    hipStream_t s = h->stream;
    EL_HIP(h, hipMemsetAsync(o.cnt.p, 0, EL_NSTAT * sizeof(unsigned long long), s));
    EL_HIP(h, hipMemsetAsync(o.st.p, 0, sizeof(ElState), s));
    double* b = o.buf;
    unsigned char* fb = o.fx;
    std::vector<double*> acell(nl), dg(nl), cn(nl, nullptr);
    std::vector<unsigned char*> fxl(nl, nullptr);
    o.rhs.assign(nl, nullptr); o.xa.assign(nl, nullptr); o.xb.assign(nl, nullptr);
    for (int l = 0; l < nl; ++l) {
        const size_t m = (size_t)lev[l].nn;
        acell[l] = b; b += ncell(lev[l]);
        dg[l] = b; b += m;
        if (c_nodes) { cn[l] = b; b += m; }
        o.xa[l] = b; b += m;
        o.xb[l] = b; b += m;
        if (l) { o.rhs[l] = b; b += m; }
        else {
            o.V.x = b; b += m; o.V.r = b; b += m; o.V.q = b; b += m; o.V.p[0] = b; b += m; o.V.p[1] = b; b += m;
        }
        if (fixed) { fxl[l] = fb; fb += m; }
        lev[l].a = acell[l]; lev[l].D = dg[l]; lev[l].cn = cn[l]; lev[l].fixed = fxl[l];
    }
    o.V.partial = o.partial;
    o.V.st = o.st;
    if (c_nodes) EL_HIP(h, hipMemcpyAsync(cn[0], c_nodes, (size_t)nn * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (fixed) EL_HIP(h, hipMemcpyAsync(fxl[0], fixed, (size_t)nn, hipMemcpyDeviceToDevice, s));
    EL_LAUNCH(N, el_setup_kernel, el_blocks(nn), EL_THREADS, s, lev[0], o.F, a_cells ? (const void*)nullptr : phi, level, a_in, a_out, hmin, a_cells,
              acell[0], o.cnt.p);
    EL_HIP(h, hipGetLastError());
    unsigned long long c[EL_NSTAT] = {};
    EL_HIP(h, hipMemcpyAsync(c, o.cnt.p, sizeof(c), hipMemcpyDeviceToHost, s));
    EL_HIP(h, hipStreamSynchronize(s));
    o.nfixed = (long long)c[EL_NFIXED];
    o.nfree = nn - o.nfixed;
    // what the data is refused for: stats = {-(reason), offending entries, 0, 0}
    const int reason = c[EL_BAD_PHI] ? 1 : c[EL_BAD_A] ? 2 : c[EL_BAD_C] ? 3 : (!c[EL_NFIXED] && !c[EL_CPOS]) ? 4 : o.nfree == 0 ? 5 : 0;
    if (reason) {
        static const char* why[5] = {"lsm_elliptic_create: phi must be finite", "lsm_elliptic_create: the cell coefficients must be finite and positive",
                                     "lsm_elliptic_create: c must be finite and not negative",
                                     "lsm_elliptic_create: no fixed node and c = 0 everywhere (the problem is singular)",
                                     "lsm_elliptic_create: every node is fixed"};
        if (stats) { stats[0] = -reason; stats[1] = (int64_t)(reason == 1 ? c[EL_BAD_PHI] : reason == 2 ? c[EL_BAD_A] : reason == 3 ? c[EL_BAD_C] : 0); stats[2] = stats[3] = 0; }
        return lsm_fail(h, LSM_ERR_INVALID, why[reason - 1]);
    }
    for (int l = 1; l < nl; ++l)
        EL_LAUNCH(N, el_coarsen_kernel, el_blocks(lev[l].nn), EL_THREADS, s, lev[l - 1], lev[l], o.co[l - 1][0], o.co[l - 1][1], o.co[l - 1][2], acell[l], cn[l],
                  fxl[l]);
    for (int l = 0; l < nl; ++l) EL_LAUNCH(N, el_diag_kernel, el_blocks(lev[l].nn), EL_THREADS, s, lev[l], dg[l]);
    EL_HIP(h, hipGetLastError());
    EL_HIP(h, hipStreamSynchronize(s));
    o.lev = lev;
    o.V.z = o.precond == LSM_PRECOND_JACOBI ? o.xa[0] : o.xb[0];
    if (stats) { stats[0] = nl; stats[1] = o.nfree; stats[2] = o.nfixed; stats[3] = 0; }
    return LSM_OK;
}

int lsm_elliptic_create(LsmHandle* h, const void* phi, double level, double a_in, double a_out, const double* a_cells, double c_const, const double* c_nodes,
                        const void* fixed, int precond, LsmElliptic** out, int64_t stats[4]) {
    if (!h || !out) return h ? lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: null argument") : LSM_ERR_INVALID;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (!phi && !a_cells) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: give phi or the cell coefficients");
    const int N = h->grid.ndim;
    if (N == 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: a 1-dimensional grid is not supported (2-D and 3-D only)");
    if (h->comm) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: the handle has a communicator attached (single device only)");
    if (h->bc[N - 1][0].kind == LSM_BC_NONE || h->bc[N - 1][1].kind == LSM_BC_NONE)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: the handle is a slab of a multi-GPU grid (whole grids only)");
    for (int d = 0; d < N; ++d) {
        if (h->bc[d][0].kind == LSM_BC_PERIODIC || h->bc[d][1].kind == LSM_BC_PERIODIC)
            return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: a periodic dimension is not supported (the faces are natural)");
        if (h->nloc[d] < 3) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: at least 3 nodes per dimension");
    }
    if (!a_cells && (!(a_in > 0) || !std::isfinite(a_in) || !(a_out > 0) || !std::isfinite(a_out)))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: a_in and a_out must be finite and positive");
    if (!a_cells && !std::isfinite(level)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: level must be finite");
    if (!c_nodes && (!(c_const >= 0) || !std::isfinite(c_const))) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: c must be finite and not negative");
    if (precond != LSM_PRECOND_MG && precond != LSM_PRECOND_JACOBI) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: unknown preconditioner");
    (void)hipSetDevice(h->device);
    EllipticObject* o = new EllipticObject();
    o->precond = precond;
    const int r = el_create(h, *o, phi, level, a_in, a_out, a_cells, c_const, c_nodes, (const unsigned char*)fixed, stats);
    if (r != LSM_OK) { delete o; return r; }
    *out = new LsmElliptic{h, o};
    return LSM_OK;
}

int lsm_elliptic_apply(LsmElliptic* s, const double* x, double* y) {
    if (!s) return LSM_ERR_INVALID;
    if (!x || !y || x == y) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_apply: x and y must be two arrays");
    const ElLevel& L = s->o->lev[0];
    EL_LAUNCH(s->o->N, el_apply_kernel, el_blocks(L.nn), EL_THREADS, s->h->stream, L, x, y);
    EL_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elliptic_cells(LsmElliptic* s, double* a_out_cells) {
    if (!s) return LSM_ERR_INVALID;
    if (!a_out_cells) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_cells: null argument");
    const ElLevel& L = s->o->lev[0];
    size_t m = 1;
    for (int d = 0; d < s->o->N; ++d) m *= (size_t)(L.n[d] - 1);
    EL_HIP(s->h, hipMemcpyAsync(a_out_cells, L.a, m * sizeof(double), hipMemcpyDeviceToDevice, s->h->stream));
    return LSM_OK;
}

int lsm_elliptic_energy(LsmElliptic* s, const void* u, void* e_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!u || !e_out || u == e_out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_energy: u and e_out must be two fields");
    const ElLevel& L = s->o->lev[0];
    EL_LAUNCH(s->o->N, el_energy_kernel, el_blocks(L.nn), EL_THREADS, s->h->stream, L, s->o->F, u, e_out);
    EL_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elliptic_compliance(LsmElliptic* s, const double* f, const void* u, double* out) {
    if (!s) return LSM_ERR_INVALID;
    if (!f || !u || !out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_compliance: null argument");
    EllipticObject& o = *s->o;
    const ElLevel& L = o.lev[0];
    hipStream_t st = s->h->stream;
    EL_LAUNCH(o.N, el_compliance_kernel, el_blocks(L.nn), EL_THREADS, st, L, o.F, f, u, o.partial.p, o.st.p);
    EL_HIP(s->h, hipGetLastError());
    EL_HIP(s->h, hipMemcpyAsync(o.h_st, o.st, sizeof(ElState), hipMemcpyDeviceToHost, st));
    EL_HIP(s->h, hipStreamSynchronize(st));
    double vol = 1.0;
    for (int d = 0; d < o.N; ++d) vol *= L.h[d];
    *out = vol * o.h_st.p->out;
    return LSM_OK;
}

int lsm_elliptic_solve(LsmElliptic* s, const double* f, void* u, double rtol, int max_iters, int* iters_out, double* relres_out, void* stream) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    if (!f || !u) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_solve: null argument");
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_solve: rtol must be positive and max_iters at least 1");
    EllipticObject& o = *s->o;
    const int N = o.N;
    const ElLevel& L = o.lev[0];
    const int jac = o.precond == LSM_PRECOND_JACOBI;
    (void)hipSetDevice(h->device);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    ElState s0;
    memset(&s0, 0, sizeof(s0));
    s0.rtol2 = rtol * rtol;
    s0.max_iters = max_iters;
    EL_HIP(h, hipMemcpyAsync(o.st, &s0, sizeof(s0), hipMemcpyHostToDevice, st));
    const unsigned nb = el_blocks(L.nn);
    EL_LAUNCH(N, el_init_kernel, nb, EL_THREADS, st, L, o.F, o.V, f, (const void*)u, jac);
    EL_HIP(h, hipGetLastError());
    // iterations in chunks: the first as long as the last solve took, then doubling
    int enq = 0;
    int chunk = std::max(4, o.last_iters + 1);
    for (;;) {
        const int k = std::min(chunk, max_iters - enq);
        for (int it = 0; it < k; ++it, ++enq) {
            const int par = enq & 1;
            if (!jac) el_vcycle(o, st);
            EL_LAUNCH(N, el_k1_kernel, nb, EL_THREADS, st, L, o.V, par);
            if (jac) hipLaunchKernelGGL(el_k2_kernel<1>, dim3(nb), dim3(EL_THREADS), 0, st, L, o.V, par);
            else hipLaunchKernelGGL(el_k2_kernel<0>, dim3(nb), dim3(EL_THREADS), 0, st, L, o.V, par);
        }
        EL_HIP(h, hipGetLastError());
        EL_HIP(h, hipMemcpyAsync(o.h_st, o.st, sizeof(ElState), hipMemcpyDeviceToHost, st));
        EL_HIP(h, hipStreamSynchronize(st));
        if (o.h_st.p->status != EL_RUN || enq >= max_iters) break;
        chunk = std::min(2 * chunk, 64);
    }
    const ElState S = *o.h_st;
    const double rel = S.bb > 0 ? std::sqrt(S.rr / S.bb) : (S.rr == 0 ? 0.0 : std::sqrt(S.rr));
    if (iters_out) *iters_out = S.iters;
    if (relres_out) *relres_out = rel;
    if (S.status == EL_BREAK_INPUT) {
        char msg[200];
        snprintf(msg, sizeof(msg), "lsm_elliptic_solve: f and u must be finite (%llu entries are not); u is unchanged", S.nonfinite);
        return lsm_fail(h, LSM_ERR_INVALID, msg);
    }
    if (S.status != EL_CONVERGED) {
        char msg[320];
        const char* why = S.status == EL_MAXITER || S.status == EL_RUN ? "no convergence within max_iters"
                          : S.status == EL_BREAK_SIGMA ? "PCG breakdown (p·Ap not positive)"
                                                       : "PCG breakdown (r·Mr not positive, or a non-finite residual)";
        snprintf(msg, sizeof(msg), "lsm_elliptic_solve: %s: %d iterations, relative residual %.3e (rtol %.3e); u is unchanged", why, S.iters, rel, rtol);
        return lsm_fail(h, LSM_ERR_NOT_CONVERGED, msg);
    }
    o.last_iters = S.iters;
    EL_LAUNCH(N, el_store_kernel, nb, EL_THREADS, st, L, o.F, (const double*)o.V.x, u);
    EL_HIP(h, hipGetLastError());
    EL_HIP(h, hipStreamSynchronize(st));
    return LSM_OK;
}

void lsm_elliptic_destroy(LsmElliptic* s) {
    if (!s) return;
    delete s->o;
    delete s;
}
