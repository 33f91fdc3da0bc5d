// mg_pcg.h — the multigrid-preconditioned conjugate gradients that lsm_elliptic.hip and lsm_elastic.hip share: the device state and
// its scalar updates, K2, the V-cycle's kernels and driver, the hierarchy's shapes, the host's iteration loop and outcome report.
// An operator's file brings a level struct (below: "Level") with its apply; everything here is written once over it.  Both files
// are built with -ffp-contract=off and this header inherits that.  DESIGN.md §7.17 (scalar), §7.18 (elasticity).
//
// Vectors are fp64 and component-major: x[i·nn + id], id = i0 + n0·(i1 + n1·i2); the scalar problem has one component.
//
// One PCG iteration:
//   [z = M r, ρ' = r·z, β = ρ'/ρ]   the V-cycle, whose last sweep carries the dot product — or, for M = D⁻¹, part of K2
//   K1  p' = z + β p,  q = A p',  σ = p'·q   → α = ρ/σ   (the operator's own kernels: how p is updated differs)
//   K2  x += α p',  r −= α q,  r·r → converged?  (Jacobi: z = r/D, ρ' = r·z as well)
// A batched solve (MANY = 1 on the kernels, mg_vcycle<1>) runs K ≤ MG_MAXCOLS right-hand sides of one operator in the same launches: the
// column is blockIdx.z.  Every vector of a level is the single solve's layout repeated at the column stride comps·nn, every column has
// its own MgState (tickets included) and its own 4·MG_MAXB partials, and the launch shape in x is the single solve's, so a column runs
// the single solve's arithmetic in its order: the same bits.  A column that has left MG_RUN is skipped by its own workgroups.  With
// MANY = 0 the kernels are the single solve's, token for token.
// Reductions by wave.h's block_reduce_ordered: one partial per workgroup, the last workgroup to draw a ticket sums them in
// workgroup order and updates the scalars; every kernel returns at once when the device status is set, the host enqueues
// iterations in chunks and reads the status once per chunk.
//
// The V-cycle (from zero, for A x = r on the free components; ω the level's damping):
//   per level but the coarsest:  x = ω r/D;  x ← x + ω (r − A x)/D;  r_c = Pᵀ(r − A x)/2^k (the fine residual written once into
//   the level's free smoother buffer, then gathered);  …coarser levels…;  x += P x_c (one kernel, in place);  two more sweeps.
//   The coarsest level (≤ 5 nodes per axis, so ≤ 125 nodes): 16 sweeps from zero in ONE single-workgroup kernel, x in LDS.
//   Fixed components: residuals and corrections are zero there; a coarse node takes the mask of fine node 2J.
//
// What a Level gives:
//   n[3], nn, h[3], D                      the shape, the spacings, the diagonal (component-major)
//   using Vec                              the solver's vectors: MgVec and the search direction(s)
//   static constexpr int comps(int N)      components per node
//   bool fixed(id, comp), double omega()   the mask, the damping
//   static launch_resid(N, nb, stream, L, r, x, res, st)   launches the level's residual kernel: mg_resid_kernel, or its own
//   apply<N, MASK>(id, I, x, stride, out)  the comps(N) rows of the eliminated operator at node id from x[j·stride + q].  MASK: x may
//                                          hold anything on fixed components (they are not read); without it x holds zero there.
//   optional: static constexpr bool wraps = true, with launch_gather and launch_prolong (see mg_wraps below): a grid that wraps;
//             its index arithmetic, its transfers and the Levels' common base are cell_problem.h's
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "lsm_handle.h"
#include "wave.h"

namespace lsm {

static const int MG_THREADS = 256;
static const int MG_MAXB = 2048;
static const int MG_NCOARSE = 16;
static const int MG_MAXCOLS = 8;      // the columns of a batched solve (MANY, below)
enum { MG_RUN = 0, MG_CONVERGED = 1, MG_MAXITER = 2, MG_BREAK_INPUT = -1, MG_BREAK_SIGMA = -2, MG_BREAK_RHO = -3 };

struct MgState {
    double rho, alpha, beta, bb, rr, rtol2, out;
    int status, iters, max_iters, first;
    unsigned long long nonfinite;
    unsigned ticket[4];
};

struct MgVec {
    double *x, *r, *q, *z;   // z: where the preconditioner leaves M r
    double* partial;
    MgState* st;
};

// where a field of the handle lives (padded layout), for the kernels that read or write one
struct MgField { long long s1, s2, origin; int f32; };

template <int N>
__device__ __forceinline__ void mg_coords(const int n[3], int id, int I[3]) {
    I[0] = id % n[0];
    const int r = id / n[0];
    I[1] = N > 2 ? r % n[1] : r;
    I[2] = N > 2 ? r / n[1] : 0;
}
__device__ __forceinline__ long long mg_padded(const MgField& F, const int I[3]) { return F.origin + I[0] + I[1] * F.s1 + I[2] * F.s2; }
__device__ __forceinline__ bool mg_finite(double x) { return x - x == 0.0; }
// cell C of a level with n nodes per axis: n−1 cells per axis, axis 0 fastest
template <int N>
__device__ __forceinline__ int mg_cell_index(const int n[3], const int C[3]) { return C[0] + (n[0] - 1) * (C[1] + (N > 2 ? (n[1] - 1) * C[2] : 0)); }
template <int N>
__device__ __forceinline__ double mg_mass(const int n[3], const int I[3]) {
    double m = 1.0;
#pragma unroll
    for (int d = 0; d < N; ++d)
        if (I[d] == 0 || I[d] == n[d] - 1) m = m * 0.5;
    return m;
}

#define MG_LOOP(id, nn) for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < (nn); id += gridDim.x * blockDim.x)

// ---- the scalars, by thread 0 of the workgroup that finishes a reduction
// after the init pass.  red: ‖b_free‖², ‖r₀‖², r·z, non-finite entries (a count below 2^53: exact)
__device__ __forceinline__ void mg_init_tail(MgState& S, const double red[4], int jac) {
    S.bb = red[0] > 0.0 ? red[0] : red[1];      // f ≡ 0 on the free components: the norm of the eliminated right-hand side
    S.rr = red[1];
    S.rho = red[2];
    S.alpha = 0.0; S.beta = 0.0;
    S.iters = 0;
    S.first = 1;
    S.nonfinite = (unsigned long long)red[3];
    if (red[3] > 0.0 || !mg_finite(red[0]) || !mg_finite(red[1])) S.status = MG_BREAK_INPUT;
    else if (red[1] <= S.rtol2 * S.bb) S.status = MG_CONVERGED;
    else if (jac && !(red[2] > 0.0)) S.status = MG_BREAK_RHO;
    else S.status = MG_RUN;
    if (jac) S.first = 0;
}
// after K1: α = ρ/σ
__device__ __forceinline__ void mg_k1_tail(MgState& S, double sigma) {
    const double alpha = S.rho / sigma;
    if (!(sigma > 0.0) || !mg_finite(alpha)) { S.status = MG_BREAK_SIGMA; return; }
    S.alpha = alpha;
}
// after K2.  red: r·r, r·z
template <int JAC>
__device__ __forceinline__ void mg_k2_tail(MgState& S, const double red[2]) {
    S.iters += 1;
    S.rr = red[0];
    if (red[0] <= S.rtol2 * S.bb) { S.status = MG_CONVERGED; return; }
    if (!mg_finite(red[0])) { S.status = MG_BREAK_RHO; return; }
    if (JAC) {
        if (!(red[1] > 0.0) || !mg_finite(red[1])) { S.status = MG_BREAK_RHO; return; }
        S.beta = red[1] / S.rho;
        S.rho = red[1];
    }
    if (S.iters >= S.max_iters) S.status = MG_MAXITER;
}
// after z = M r of the V-cycle: ρ' = r·z, β = ρ'/ρ (0 the first time)
__device__ __forceinline__ void mg_rho_update(MgState& S, double rz) {
    if (!(rz > 0.0) || !mg_finite(rz)) { S.status = MG_BREAK_RHO; return; }
    S.beta = S.first ? 0.0 : rz / S.rho;
    S.rho = rz;
    S.first = 0;
}

// K2 over the nt unknowns: x += α p, r −= α q, r·r → converged?; JAC: z = r/D, ρ' = r·z, β = ρ'/ρ
template <int JAC, int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) mg_k2_kernel(const double* __restrict__ D, int nt, MgVec V, const double* __restrict__ p) {
    if constexpr (MANY) {
        const size_t c = blockIdx.z, at = c * (size_t)nt;
        V.x += at; V.r += at; V.q += at; V.z += at; p += at;
        V.partial += c * (4 * MG_MAXB);
        V.st += c;
    }
    if (V.st->status != MG_RUN) return;
    const double alpha = V.st->alpha;
    double red[2] = {0.0, 0.0};
    MG_LOOP(k, nt) {
        V.x[k] = V.x[k] + alpha * p[k];
        const double r = V.r[k] - alpha * V.q[k];
        V.r[k] = r;
        red[0] += r * r;
        if (JAC) {
            const double z = r / D[k];      // r is zero on the fixed components
            V.z[k] = z;
            red[1] += r * z;
        }
    }
    if (!block_reduce_ordered<2, MG_THREADS>(red, V.partial, &V.st->ticket[2]) || threadIdx.x != 0) return;
    mg_k2_tail<JAC>(*V.st, red);
}

// ---- a coarse cell from the fine ones: the mean of the cells {2J, 2J+1} per coarsened axis, ascending; scale = 2^−(coarsened axes)
template <int N>
__device__ __forceinline__ double mg_cell_average(const double* __restrict__ af, const int nf[3], const int J[3], const int co[3], double scale) {
    double s = 0.0;
    bool first = true;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {
        int C[3] = {0, 0, 0};
        bool use = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            const int b = (m >> d) & 1;
            if (!co[d] && b) use = false;
            C[d] = co[d] ? 2 * J[d] + b : J[d];
        }
        if (!use) continue;
        const double v = af[mg_cell_index<N>(nf, C)];
        s = first ? v : s + v;
        first = false;
    }
    return s * scale;
}
__device__ __forceinline__ double mg_coarsen_scale(int k) { return k == 1 ? 0.5 : k == 2 ? 0.25 : 0.125; }

// ---- the V-cycle's kernels (any level)
// first sweep from zero: x = ω r/D (NC: the components per node)
template <int NC, class Level, int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) mg_smooth0_kernel(Level L, const double* __restrict__ r, double* __restrict__ x, const MgState* st) {
    if constexpr (MANY) {
        const size_t at = (size_t)blockIdx.z * NC * L.nn;
        r += at; x += at;
        st += blockIdx.z;
    }
    if (st->status != MG_RUN) return;
    const int nn = L.nn;
    MG_LOOP(id, nn) {
#pragma unroll
        for (int i = 0; i < NC; ++i) x[i * nn + id] = L.fixed(id, i) ? 0.0 : (L.omega() * r[i * nn + id]) / L.D[i * nn + id];
    }
}
// xn = x + ω (r − A x)/D; DOT (the cycle's last sweep on level 0): r·xn and the scalars.  (Here and below: a node whose only
// component is fixed needs no row.)
template <int N, int DOT, class Level, int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) mg_smooth_kernel(Level L, const double* __restrict__ r, const double* __restrict__ x, double* __restrict__ xn,
                                                               double* partial, MgState* st) {
    if constexpr (MANY) {
        const size_t c = blockIdx.z, at = c * Level::comps(N) * L.nn;
        r += at; x += at; xn += at;
        partial += c * (4 * MG_MAXB);
        st += c;
    }
    if (st->status != MG_RUN) return;
    constexpr int NC = Level::comps(N);
    const int nn = L.nn;
    double red[1] = {0.0};
    MG_LOOP(id, nn) {
        bool fx[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) fx[i] = L.fixed(id, i);
        double v[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) v[i] = 0.0;
        if (NC > 1 || !fx[0]) {
            int I[3];
            mg_coords<N>(L.n, id, I);
            double out[NC];
            L.template apply<N, true>(id, I, x, nn, out);
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if (!fx[i]) {
                    const double ri = r[i * nn + id];
                    v[i] = x[i * nn + id] + (L.omega() * (ri - out[i])) / L.D[i * nn + id];
                    if (DOT) red[0] += ri * v[i];
                }
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) xn[i * nn + id] = v[i];
    }
    if (DOT) {
        if (!block_reduce_ordered<1, MG_THREADS>(red, partial, &st->ticket[3]) || threadIdx.x != 0) return;
        mg_rho_update(*st, red[0]);
    }
}
// the fine residual, zero on the fixed components, written once (into the level's free smoother buffer), then gathered
template <int N, class Level, int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) mg_resid_kernel(Level L, const double* __restrict__ r, const double* __restrict__ x, double* __restrict__ res,
                                                              const MgState* st) {
    if constexpr (MANY) {
        const size_t at = (size_t)blockIdx.z * Level::comps(N) * L.nn;
        r += at; x += at; res += at;
        st += blockIdx.z;
    }
    if (st->status != MG_RUN) return;
    constexpr int NC = Level::comps(N);
    const int nn = L.nn;
    MG_LOOP(id, nn) {
        bool fx[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) fx[i] = L.fixed(id, i);
        double out[NC];
        if (NC > 1 || !fx[0]) {
            int I[3];
            mg_coords<N>(L.n, id, I);
            L.template apply<N, true>(id, I, x, nn, out);
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) res[i * nn + id] = fx[i] ? 0.0 : r[i * nn + id] - out[i];
    }
}
// r_c = Pᵀ res / 2^k per component (blockIdx.y): a coarse node gathers from the fine nodes 2J + o, o ∈ {−1, 0, 1} per coarsened axis
template <int N, class Level, int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) mg_gather_kernel(Level Lf, Level Lc, int co0, int co1, int co2, const double* __restrict__ res,
                                                               double* __restrict__ rc, const MgState* st) {
    if constexpr (MANY) {
        const size_t c = blockIdx.z;
        res += c * Level::comps(N) * Lf.nn;
        rc += c * Level::comps(N) * Lc.nn;
        st += c;
    }
    if (st->status != MG_RUN) return;
    const int co[3] = {co0, co1, co2};
    const double scale = mg_coarsen_scale(co0 + co1 + co2);
    const int comp = blockIdx.y;
    res += (size_t)comp * Lf.nn;
    rc += (size_t)comp * Lc.nn;
    MG_LOOP(id, Lc.nn) {
        double acc = 0.0;
        if (!Lc.fixed(id, comp)) {
            int J[3];
            mg_coords<N>(Lc.n, id, J);
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
                if (use) acc += w * res[I[0] + Lf.n[0] * (I[1] + (N > 2 ? Lf.n[1] * I[2] : 0))];     // zero on fixed fine components
            }
        }
        rc[id] = acc * scale;
    }
}
// x += P x_c on the free fine components, per component (blockIdx.y)
template <int N, class Level, int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) mg_prolong_kernel(Level Lf, Level Lc, int co0, int co1, int co2, const double* __restrict__ xc,
                                                                double* __restrict__ x, const MgState* st) {
    if constexpr (MANY) {
        const size_t c = blockIdx.z;
        xc += c * Level::comps(N) * Lc.nn;
        x += c * Level::comps(N) * Lf.nn;
        st += c;
    }
    if (st->status != MG_RUN) return;
    const int co[3] = {co0, co1, co2};
    const int comp = blockIdx.y;
    xc += (size_t)comp * Lc.nn;
    x += (size_t)comp * Lf.nn;
    MG_LOOP(id, Lf.nn) {
        if (Lf.fixed(id, comp)) continue;
        int I[3];
        mg_coords<N>(Lf.n, id, I);
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
// the coarsest level (≤ 128 nodes): MG_NCOARSE sweeps from zero in one workgroup, x in LDS (component stride 128), double-buffered
template <int N, int DOT, class Level, int MANY = 0>
__global__ void __launch_bounds__(128) mg_coarsest_kernel(Level L, const double* __restrict__ r, double* __restrict__ x, MgState* st) {
    constexpr int NC = Level::comps(N);
    __shared__ double xs[2][NC * 128];
    __shared__ double red[2];
    if constexpr (MANY) {      // one workgroup per column
        const size_t at = (size_t)blockIdx.z * NC * L.nn;
        r += at; x += at;
        st += blockIdx.z;
    }
    if (st->status != MG_RUN) return;
    const int id = threadIdx.x, nn = L.nn;
    const bool node = id < nn;
    int I[3] = {0, 0, 0};
    if (node) mg_coords<N>(L.n, id, I);
    bool on[NC];
    double ri[NC], Di[NC], v[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        on[i] = node && !L.fixed(id, i);
        ri[i] = on[i] ? r[i * nn + id] : 0.0;
        Di[i] = on[i] ? L.D[i * nn + id] : 1.0;
        v[i] = on[i] ? (L.omega() * ri[i]) / Di[i] : 0.0;
    }
    int cur = 0;
    for (int s = 1; s < MG_NCOARSE; ++s) {
#pragma unroll
        for (int i = 0; i < NC; ++i) xs[cur][i * 128 + id] = v[i];
        __syncthreads();
        if (node && (NC > 1 || on[0])) {
            double out[NC];
            L.template apply<N, false>(id, I, xs[cur], 128, out);     // fixed components hold zero
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if (on[i]) v[i] = v[i] + (L.omega() * (ri[i] - out[i])) / Di[i];
        }
        cur ^= 1;
    }
    if (node) {
#pragma unroll
        for (int i = 0; i < NC; ++i) x[i * nn + id] = v[i];
    }
    if (DOT) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < NC; ++i) t += ri[i] * v[i];
        const double s = wave_sum(t);
        if ((id & 63) == 0) red[id >> 6] = s;
        __syncthreads();
        if (id == 0) mg_rho_update(*st, red[0] + red[1]);
    }
}

// ---- host side
static unsigned mg_blocks(long long n) { return (unsigned)std::min<long long>((n + MG_THREADS - 1) / MG_THREADS, MG_MAXB); }

// kernel<N>, kernel<N, A>, kernel<N, A, B> for the handle's N
#define MG_LAUNCH_AS(N, k2, k3, grid, block, stream, ...)                                  \
    do {                                                                                   \
        if ((N) == 2) hipLaunchKernelGGL(k2, dim3(grid), dim3(block), 0, stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(k3, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);      \
    } while (0)
#define MG_LAUNCH(N, kernel, ...) MG_LAUNCH_AS(N, kernel<2>, kernel<3>, __VA_ARGS__)
#define MG_LAUNCH2(N, kernel, A, ...) MG_LAUNCH_AS(N, (kernel<2, A>), (kernel<3, A>), __VA_ARGS__)
#define MG_LAUNCH3(N, kernel, A, B, ...) MG_LAUNCH_AS(N, (kernel<2, A, B>), (kernel<3, A, B>), __VA_ARGS__)
#define MG_LAUNCH4(N, kernel, A, B, C, ...) MG_LAUNCH_AS(N, (kernel<2, A, B, C>), (kernel<3, A, B, C>), __VA_ARGS__)

template <class Level>
struct MgSolver {
    int N = 0, precond = 0, last_iters = 0;
    int cols = 1;                        // the columns that the vectors, the states and the partials are allocated for (a batch workspace: > 1 possible)
    int co[32][3];                       // co[l]: the axes that coarsen from level l to l+1
    std::vector<Level> lev;
    std::vector<double*> rhs, xa, xb;    // per level ≥ 1: right-hand side and the two smoother buffers; level 0: xa, xb only
    typename Level::Vec V;
    MgField F;
    long long nfree = 0, nfixed = 0;
    DevBuf<double> buf, partial;
    DevBuf<unsigned char> fx;
    DevBuf<MgState> st;
    DevBuf<unsigned long long> cnt;
    PinnedBuf<MgState> h_st;
};

// the hierarchy's shapes from the handle's grid: n, h, nn of every level and co.  Axis d coarsens while n_d > 5, to (n_d+1)/2 nodes
// with 2h; the hierarchy ends when no axis coarsens (31 levels at most).  L0: the operator's own fields of level 0, copied down.
// Returns the nodes of level 0 and leaves lev empty when there are max_nodes or more; hmin: the smallest spacing of level 0
template <class Level>
static long long mg_shapes(const LsmHandle* h, Level L0, long long max_nodes, std::vector<Level>& lev, int co[32][3], double& hmin) {
    const int N = h->grid.ndim;
    long long nn = 1;
    hmin = INFINITY;
    for (int d = 0; d < 3; ++d) {
        L0.n[d] = d < N ? h->nloc[d] : 1;
        L0.h[d] = d < N ? h->h[d] : 1.0;
        nn *= L0.n[d];
        if (d < N) hmin = std::min(hmin, L0.h[d]);
    }
    lev.clear();
    if (nn >= max_nodes) return nn;
    L0.nn = (int)nn;
    lev.push_back(L0);
    for (;;) {
        const Level& f = lev.back();
        Level c = f;
        bool any = false;
        const int l = (int)lev.size() - 1;
        c.nn = 1;
        for (int d = 0; d < 3; ++d) {
            co[l][d] = d < N && f.n[d] > 5;
            if (co[l][d]) {
                any = true;
                c.n[d] = (f.n[d] + 1) / 2;
                c.h[d] = f.h[d] * 2.0;
            }
            c.nn *= c.n[d];
        }
        if (!any || lev.size() >= 31) break;
        lev.push_back(c);
    }
    return nn;
}

template <class Level>
static size_t mg_ncells(int N, const Level& L) {
    size_t m = 1;
    for (int d = 0; d < N; ++d) m *= (size_t)(L.n[d] - 1);
    return m;
}

// the reduction partials, the device state with its pinned copy and nstat setup counters, all zero
template <class Level>
static int mg_alloc_scalars(LsmHandle* h, MgSolver<Level>& o, int nstat, hipStream_t s) {
    LSM_HIP(h, o.partial.alloc(4 * MG_MAXB * sizeof(double)));
    LSM_HIP(h, o.st.alloc(sizeof(MgState)));
    LSM_HIP(h, o.cnt.alloc(nstat * sizeof(unsigned long long)));
    LSM_HIP(h, o.h_st.alloc(sizeof(MgState)));
    LSM_HIP(h, hipMemsetAsync(o.cnt.p, 0, nstat * sizeof(unsigned long long), s));
    LSM_HIP(h, hipMemsetAsync(o.st.p, 0, sizeof(MgState), s));
    o.V.partial = o.partial;
    o.V.st = o.st;
    return LSM_OK;
}

// A Level whose grid wraps (cell_problem.h's CpLevel) declares `static constexpr bool wraps = true` and launches the wrapping
// transfers (cell_problem.h's mg_wrap_gather_kernel, mg_wrap_prolong_kernel) from
//   static launch_gather(N, stream, Lf, Lc, co, res, rc, st),  static launch_prolong(N, stream, Lf, Lc, co, xc, x, st);
// every other Level takes mg_gather_kernel and mg_prolong_kernel, as before.
template <class Level, class = void>
struct mg_wraps : std::false_type {};
template <class Level>
struct mg_wraps<Level, std::void_t<decltype(Level::wraps)>> : std::true_type {};

// z = M r0 for M = one V-cycle, into xb[0]; the last kernel leaves ρ and β.  MANY: the same for the first `cols` columns of a batch
// workspace (a Level that takes part has launch_resid_many); the launches are the single cycle's with the columns as the grid's z
template <int MANY = 0, class Level>
static void mg_vcycle(MgSolver<Level>& o, const double* r0, hipStream_t s, int cols = 1) {
    static_assert(!MANY || !mg_wraps<Level>::value, "the wrapping transfers have no column dimension");
    const int N = o.N, nl = (int)o.lev.size(), nc = Level::comps(N);
    const unsigned nz = (unsigned)cols;
    MgState* st = o.st;
    for (int l = 0; l + 1 < nl; ++l) {
        const Level& L = o.lev[l];
        const double* r = l == 0 ? r0 : o.rhs[l];
        const unsigned nb = mg_blocks(L.nn);
        MG_LAUNCH_AS(N, (mg_smooth0_kernel<Level::comps(2), Level, MANY>), (mg_smooth0_kernel<Level::comps(3), Level, MANY>), dim3(nb, 1, nz), MG_THREADS, s, L, r, o.xa[l],
                     (const MgState*)st);
        MG_LAUNCH4(N, mg_smooth_kernel, 0, Level, MANY, dim3(nb, 1, nz), MG_THREADS, s, L, r, (const double*)o.xa[l], o.xb[l], o.partial.p, st);
        if constexpr (MANY) Level::launch_resid_many(N, nb, nz, s, L, r, o.xb[l], o.xa[l], st);
        else Level::launch_resid(N, nb, s, L, r, o.xb[l], o.xa[l], st);      // xa is free until the post-smoothing
        if constexpr (mg_wraps<Level>::value) Level::launch_gather(N, s, L, o.lev[l + 1], o.co[l], (const double*)o.xa[l], o.rhs[l + 1], (const MgState*)st);
        else
            MG_LAUNCH3(N, mg_gather_kernel, Level, MANY, dim3(mg_blocks(o.lev[l + 1].nn), nc, nz), MG_THREADS, s, L, o.lev[l + 1], o.co[l][0], o.co[l][1], o.co[l][2],
                       (const double*)o.xa[l], o.rhs[l + 1], (const MgState*)st);
    }
    {
        const int l = nl - 1;
        const Level& L = o.lev[l];
        const double* r = l == 0 ? r0 : o.rhs[l];
        if (L.nn > 128) {
            // a coarsest level too large for one workgroup (a wrapping grid with an odd axis; the other Levels refuse it when they
            // are created): the same MG_NCOARSE sweeps, the same arithmetic, as launches of the smoother; the last one lands in xb
            static_assert(MG_NCOARSE % 2 == 0, "the sweeps alternate xa, xb and end in xb");
            const unsigned nb = mg_blocks(L.nn);
            MG_LAUNCH_AS(N, (mg_smooth0_kernel<Level::comps(2), Level, MANY>), (mg_smooth0_kernel<Level::comps(3), Level, MANY>), dim3(nb, 1, nz), MG_THREADS, s, L, r, o.xa[l],
                         (const MgState*)st);
            for (int k = 1; k < MG_NCOARSE; ++k) {
                const double* from = (k & 1) ? o.xa[l] : o.xb[l];
                double* to = (k & 1) ? o.xb[l] : o.xa[l];
                if (l == 0 && k == MG_NCOARSE - 1) MG_LAUNCH4(N, mg_smooth_kernel, 1, Level, MANY, dim3(nb, 1, nz), MG_THREADS, s, L, r, from, to, o.partial.p, st);
                else MG_LAUNCH4(N, mg_smooth_kernel, 0, Level, MANY, dim3(nb, 1, nz), MG_THREADS, s, L, r, from, to, o.partial.p, st);
            }
        } else if (l == 0) MG_LAUNCH4(N, mg_coarsest_kernel, 1, Level, MANY, dim3(1, 1, nz), 128, s, L, r, o.xb[l], st);
        else MG_LAUNCH4(N, mg_coarsest_kernel, 0, Level, MANY, dim3(1, 1, nz), 128, s, L, r, o.xb[l], st);
    }
    for (int l = nl - 2; l >= 0; --l) {
        const Level& L = o.lev[l];
        const double* r = l == 0 ? r0 : o.rhs[l];
        const unsigned nb = mg_blocks(L.nn);
        if constexpr (mg_wraps<Level>::value) Level::launch_prolong(N, s, L, o.lev[l + 1], o.co[l], (const double*)o.xb[l + 1], o.xb[l], (const MgState*)st);
        else
            MG_LAUNCH3(N, mg_prolong_kernel, Level, MANY, dim3(nb, nc, nz), MG_THREADS, s, L, o.lev[l + 1], o.co[l][0], o.co[l][1], o.co[l][2], (const double*)o.xb[l + 1],
                       o.xb[l], (const MgState*)st);
        MG_LAUNCH4(N, mg_smooth_kernel, 0, Level, MANY, dim3(nb, 1, nz), MG_THREADS, s, L, r, (const double*)o.xb[l], o.xa[l], o.partial.p, st);
        if (l == 0) MG_LAUNCH4(N, mg_smooth_kernel, 1, Level, MANY, dim3(nb, 1, nz), MG_THREADS, s, L, r, (const double*)o.xa[l], o.xb[l], o.partial.p, st);
        else MG_LAUNCH4(N, mg_smooth_kernel, 0, Level, MANY, dim3(nb, 1, nz), MG_THREADS, s, L, r, (const double*)o.xa[l], o.xb[l], o.partial.p, st);
    }
}

// the device state of a new solve (of its first `cols` columns)
template <class Level>
static int mg_reset(LsmHandle* h, MgSolver<Level>& o, double rtol, int max_iters, hipStream_t st, int cols = 1) {
    MgState s0[MG_MAXCOLS];
    memset(s0, 0, sizeof(s0));
    for (int c = 0; c < cols; ++c) {
        s0[c].rtol2 = rtol * rtol;
        s0[c].max_iters = max_iters;
    }
    LSM_HIP(h, hipMemcpyAsync(o.st, s0, cols * sizeof(MgState), hipMemcpyHostToDevice, st));
    return LSM_OK;
}

// iterations in chunks: the first as long as the last solve took, then doubling up to 64; one status read per chunk.
// enqueue(k) enqueues iteration k; the states of the `cols` columns are left in o.h_st, and the loop ends when none of them is running
template <class Level, class Enqueue>
static int mg_iterate(LsmHandle* h, MgSolver<Level>& o, int max_iters, hipStream_t st, Enqueue enqueue, int cols = 1) {
    int enq = 0;
    int chunk = std::max(4, o.last_iters + 1);
    for (;;) {
        const int k = std::min(chunk, max_iters - enq);
        for (int it = 0; it < k; ++it, ++enq) enqueue(enq);
        LSM_HIP(h, hipGetLastError());
        LSM_HIP(h, hipMemcpyAsync(o.h_st, o.st, cols * sizeof(MgState), hipMemcpyDeviceToHost, st));
        LSM_HIP(h, hipStreamSynchronize(st));
        bool running = false;
        for (int c = 0; c < cols; ++c) running = running || o.h_st.p[c].status == MG_RUN;
        if (!running || enq >= max_iters) break;
        chunk = std::min(2 * chunk, 64);
    }
    return LSM_OK;
}

static double mg_relres(const MgState& S) { return S.bb > 0 ? std::sqrt(S.rr / S.bb) : (S.rr == 0 ? 0.0 : std::sqrt(S.rr)); }

// what the solve came to, from o.h_st: the iterations, the relative residual, and LSM_OK only when it converged (fn: the caller's name).
// col ≥ 0: of that column of a batched solve, which the message then names
template <class Level>
static int mg_report(LsmHandle* h, MgSolver<Level>& o, const char* fn, double rtol, int* iters_out, double* relres_out, int col = -1) {
    const MgState S = o.h_st.p[col < 0 ? 0 : col];
    const double rel = mg_relres(S);
    char who[24] = "";
    if (col >= 0) snprintf(who, sizeof(who), " column %d:", col);
    if (iters_out) *iters_out = S.iters;
    if (relres_out) *relres_out = rel;
    if (S.status == MG_BREAK_INPUT) {
        char msg[200];
        snprintf(msg, sizeof(msg), "%s:%s f and u must be finite (%llu entries are not); u is unchanged", fn, who, S.nonfinite);
        return lsm_fail(h, LSM_ERR_INVALID, msg);
    }
    if (S.status != MG_CONVERGED) {
        char msg[320];
        const char* why = S.status == MG_MAXITER || S.status == MG_RUN ? "no convergence within max_iters"
                          : S.status == MG_BREAK_SIGMA ? "PCG breakdown (p·Ap not positive)"
                                                       : "PCG breakdown (r·Mr not positive, or a non-finite residual)";
        snprintf(msg, sizeof(msg), "%s:%s %s: %d iterations, relative residual %.3e (rtol %.3e); u is unchanged", fn, who, why, S.iters, rel, rtol);
        return lsm_fail(h, LSM_ERR_NOT_CONVERGED, msg);
    }
    o.last_iters = col < 0 ? S.iters : std::max(o.last_iters, S.iters);
    return LSM_OK;
}

}  // namespace lsm
