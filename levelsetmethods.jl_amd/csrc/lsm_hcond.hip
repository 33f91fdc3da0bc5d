// lsm_hcond.hip — homogenize_conductivity: the effective conductivity tensor K^H of −∇·(a∇u) for the periodic material whose cell is
// the box of ϕ, and its sensitivity.  lsm_elliptic.hip's edge operator with c = 0 on the torus of the grid's cells (period n − 1
// cells: node n − 1 is node 0), the N cell problems A χ^p = f^p solved by cell_problem.h over mg_pcg.h's conjugate gradients with a
// wrapping V-cycle, then one pass over the cells for the tensor.  DESIGN.md §7.24; include/lsm.h ("homogenize_conductivity") is the
// normative text, tests/_hcond_ref.py restates it.  Built with -ffp-contract=off: the cell array, A x, the loads, the cell integrands
// and the sensitivity round as numpy does.
//
// Storage.  cell_problem.h's, with one component per node and N correctors of nn doubles.
//
// What is mg_pcg.h's: the state, K2, the smoother, the coarsest kernel, the V-cycle's driver, the iteration loop, the report.  What is
// cell_problem.h's: the wrapped index arithmetic and transfers, the Level's base, the hierarchy, the allocation, the setup and its
// refusals, the PCG's start, init, direction and K1 kernels, the solves, the correctors' storage, the host tails of the tensor and
// the sensitivity, its gather, the store.  What is this file's own: the wrapping edge operator (the Level), the diagonal, the load,
// and the cell kernels.
#include <memory>

#include "cell_problem.h"

namespace lsm {

static const double HC_OMEGA = 0.8;      // lsm_elliptic.hip's damping

struct HcLevel : CpLevel<HcLevel> {
    int n[3];                     // nodes (= cells) of the torus per axis
    int nn;
    double h[3], ih2[3];
    const double* cell;           // cell coefficients
    const double* D;              // the diagonal

    static constexpr int comps(int) { return 1; }
    __device__ __forceinline__ bool fixed(int id, int) const { return id == 0; }
    __device__ __forceinline__ static double omega() { return HC_OMEGA; }
    // the operator's row at a node; x holds zero at node 0, so there is nothing to mask
    template <int N, bool MASK>
    __device__ __forceinline__ void apply(int id, const int I[3], const double* x, int stride, double out[1]) const;
};

// the 2^N cells around node I: bit d of m set: cell I_d along d, clear: cell I_d − 1, wrapped
template <int N>
__device__ __forceinline__ void hc_cells_around(const HcLevel& L, const int c[3][3], double v[1 << N]) {
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) v[m] = L.cell[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
}
// k̄ of the edge along d on side s (0: towards I − e_d, 1: towards I + e_d): (the cells with bit d = s, ascending, from +0)·2^−(N−1)
template <int N>
__device__ __forceinline__ double hc_kbar(const double v[1 << N], int d, int s) {
    double S = 0.0;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m)
        if (((m >> d) & 1) == s) S = S + v[m];
    return S * (N == 2 ? 0.5 : 0.25);
}

// (A x)_I in lsm_elliptic.hip's order: d ascending, the minus side before the plus side, from +0; xat(q) gives x at a neighbour
template <int N, class X>
__device__ __forceinline__ double hc_apply(const HcLevel& L, const int I[3], double xi, X xat) {
    int c[3][3];
    mg_wrapped<N>(L.n, I, c);
    double v[1 << N];
    hc_cells_around<N>(L, c, v);
    const int id = c[0][1] + c[1][1] + c[2][1];
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        acc = acc + (hc_kbar<N>(v, d, 0) * L.ih2[d]) * (xi - xat(id - c[d][1] + c[d][0]));
        acc = acc + (hc_kbar<N>(v, d, 1) * L.ih2[d]) * (xi - xat(id - c[d][1] + c[d][2]));
    }
    return acc;
}
template <int N, bool MASK>
__device__ __forceinline__ void HcLevel::apply(int id, const int I[3], const double* x, int, double out[1]) const {
    out[0] = hc_apply<N>(*this, I, x[id], [&](int q) { return x[q]; });
}

// ---- the diagonal: D_I = Σ_d (k̄_−·ih2_d + k̄_+·ih2_d), in the operator's order, from +0
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_diag_kernel(HcLevel L, double* __restrict__ D) {
    MG_LOOP(id, L.nn) {
        int I[3], c[3][3];
        mg_coords<N>(L.n, id, I);
        mg_wrapped<N>(L.n, I, c);
        double v[1 << N];
        hc_cells_around<N>(L, c, v);
        double acc = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            acc = acc + hc_kbar<N>(v, d, 0) * L.ih2[d];
            acc = acc + hc_kbar<N>(v, d, 1) * L.ih2[d];
        }
        D[id] = acc;
    }
}

// ---- the load of the unit gradient e_p: f_I = k̄(I → I + e_p)/h_p − k̄(I − e_p → I)/h_p
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_load_kernel(HcLevel L, int p, double* __restrict__ f) {
    MG_LOOP(id, L.nn) {
        int I[3], c[3][3];
        mg_coords<N>(L.n, id, I);
        mg_wrapped<N>(L.n, I, c);
        double v[1 << N];
        hc_cells_around<N>(L, c, v);
        double out = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d)
            if (d == p) out = hc_kbar<N>(v, d, 1) / L.h[d] - hc_kbar<N>(v, d, 0) / L.h[d];
        f[id] = out;
    }
}

// ---- y = A x on all nodes, no pin (lsm_hcond_apply)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_apply_kernel(HcLevel L, const double* __restrict__ x, double* __restrict__ y) {
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        y[id] = hc_apply<N>(L, I, x[id], [&](int q) { return x[q]; });
    }
}

// ---- the cell kernels.  On the edge along d that starts at corner a of cell C (bit d of a clear; e counts those corners ascending):
// g^p[d][e] = δ_dp + (χ^p[a + e_d] − χ^p[a])/h_d;  t^{pq}_C = (a_C·2^−(N−1))·(Σ_d Σ_e g^p[d][e]·g^q[d][e]), d ascending, within it e ascending,
// from +0
template <int N>
__device__ __forceinline__ void hc_grad(const HcLevel& L, const int node[1 << N], const double* __restrict__ chi, int p, double g[N][1 << (N - 1)]) {
#pragma unroll
    for (int d = 0; d < N; ++d) {
        int e = 0;
#pragma unroll
        for (int a = 0; a < (1 << N); ++a) {
            if ((a >> d) & 1) continue;
            g[d][e++] = (d == p ? 1.0 : 0.0) + (chi[node[a | (1 << d)]] - chi[node[a]]) / L.h[d];
        }
    }
}
template <int N>
__device__ __forceinline__ double hc_pair(double ac, const double gp[N][1 << (N - 1)], const double gq[N][1 << (N - 1)]) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d)
#pragma unroll
        for (int e = 0; e < (1 << (N - 1)); ++e) s = s + gp[d][e] * gq[d][e];
    return (ac * (N == 2 ? 0.5 : 0.25)) * s;
}

// t^{pq} of every cell, for one pair (lsm_hcond_energy_cells)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_energy_kernel(HcLevel L, const double* __restrict__ chip, const double* __restrict__ chiq, int p, int q,
                                                               double* __restrict__ out) {
    MG_LOOP(id, L.nn) {
        int C[3], node[1 << N];
        mg_coords<N>(L.n, id, C);
        mg_wrapped_corners<N>(L.n, C, node);
        double gp[N][1 << (N - 1)], gq[N][1 << (N - 1)];
        hc_grad<N>(L, node, chip, p, gp);
        hc_grad<N>(L, node, chiq, q, gq);
        out[id] = hc_pair<N>(L.cell[id], gp, gq);
    }
}

// all N(N+1)/2 sums Σ_C t^{pq}_C, p ≤ q, in one pass over the cells; entry e counts q ascending, within it p ascending.  A thread holds
// the N·N·2^(N−1) edge gradients of its cell (36 doubles in 3-D).
// SENS (lsm_hcond_sensitivity): no reduction; the same pairs in the same order, cell[C] = Σ_q Σ_{p ≤ q} (c·W[p·N + q])·t^{pq}_C from +0,
// c = 2 for p < q (W is symmetric, and t^{qp} is t^{pq} as in the mirrored tensor).
template <int N, int SENS>
__global__ void __launch_bounds__(MG_THREADS) hc_tensor_kernel(HcLevel L, const double* __restrict__ chi, const double* __restrict__ W, double* __restrict__ cell,
                                                               double* partial, unsigned* ticket, double* __restrict__ out) {
    constexpr int NP = N * (N + 1) / 2;
    const int nn = L.nn;
    double red[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) red[e] = 0.0;
    MG_LOOP(id, nn) {
        int C[3], node[1 << N];
        mg_coords<N>(L.n, id, C);
        mg_wrapped_corners<N>(L.n, C, node);
        const double ac = L.cell[id];
        double g[N][N][1 << (N - 1)];
#pragma unroll
        for (int p = 0; p < N; ++p) hc_grad<N>(L, node, chi + (size_t)p * nn, p, g[p]);
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < N; ++q)
#pragma unroll
            for (int p = 0; p <= q; ++p) {
                const double t = hc_pair<N>(ac, g[p], g[q]);
                if (SENS) acc = acc + (p < q ? 2.0 * W[p * N + q] : W[p * N + q]) * t;
                else red[q * (q + 1) / 2 + p] += t;
            }
        if (SENS) cell[id] = acc;
    }
    if (SENS) return;
    if (!block_reduce_ordered<NP, MG_THREADS>(red, partial, ticket) || threadIdx.x != 0) return;
#pragma unroll
    for (int e = 0; e < NP; ++e) out[e] = red[e];
}

// ---- host side
using HcondObject = CellProblem<HcLevel>;

static void hc_launch_load(HcondObject& o, hipStream_t st, int k, double* f) {
    const HcLevel& L = o.lev[0];
    MG_LAUNCH(o.N, hc_load_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, k, f);
}
// the tensor kernel: sens = 0 leaves the sums in o.sums, sens = 1 reads o.W and leaves a value per cell in o.cell
static void hc_launch_tensor(HcondObject& o, hipStream_t st, int sens) {
    const HcLevel& L = o.lev[0];
    const unsigned nb = mg_blocks(L.nn);
    unsigned* ticket = &o.st.p->ticket[3];
    if (sens) MG_LAUNCH2(o.N, hc_tensor_kernel, 1, dim3(nb), MG_THREADS, st, L, (const double*)o.chi, (const double*)o.W, o.cell, o.tpartial.p, ticket, o.sums);
    else MG_LAUNCH2(o.N, hc_tensor_kernel, 0, dim3(nb), MG_THREADS, st, L, (const double*)o.chi, (const double*)o.W, o.cell, o.tpartial.p, ticket, o.sums);
}

}  // namespace lsm

using namespace lsm;

struct LsmHcond { LsmHandle* h; HcondObject* o; };

static int hc_create(LsmHandle* h, HcondObject& o, const void* phi, double level, double a_in, double a_out, const double* a_cells, int64_t stats[4]) {
    std::vector<HcLevel> lev;
    double hmin;
    cp_shapes(h, o, 1LL << 29, lev, hmin);
    if (lev.empty()) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: the grid is too large (2^29 nodes at most)");
    for (HcLevel& q : lev)
        for (int d = 0; d < 3; ++d) q.ih2[d] = 1.0 / (q.h[d] * q.h[d]);
    const int N = o.K = o.N;
    CpCarve c;
    const int ra = cp_alloc(h, o, lev, 0, 0, c);
    if (ra != LSM_OK) return ra;
    return cp_setup(h, o, lev, c, "lsm_hcond_create", "coefficients", phi, level, a_in, a_out, a_cells, hmin, stats,
                    [&](const HcLevel& Ll, double* D) { MG_LAUNCH(N, hc_diag_kernel, dim3(mg_blocks(Ll.nn)), MG_THREADS, h->stream, Ll, D); });
}

int lsm_hcond_create(LsmHandle* h, const void* phi, double level, double a_in, double a_out, const double* a_cells, int precond, LsmHcond** out,
                     int64_t stats[4]) {
    const int rc = cp_create_check(h, out, stats, "lsm_hcond_create", "coefficients", "a_in", "a_out", phi, a_cells, level, a_in, a_out);
    if (rc != LSM_OK) return rc;
    const int rp = cp_check_precond(h, "lsm_hcond_create", precond);
    if (rp != LSM_OK) return rp;
    (void)hipSetDevice(h->device);
    std::unique_ptr<HcondObject> o(new HcondObject());
    o->precond = precond;
    const int r = hc_create(h, *o, phi, level, a_in, a_out, a_cells, stats);
    if (r != LSM_OK) return r;
    *out = new LsmHcond{h, o.release()};
    return LSM_OK;
}

int lsm_hcond_cells(LsmHcond* s, double* a_out_cells) { return s ? cp_cells(s->h, *s->o, "lsm_hcond_cells", a_out_cells) : LSM_ERR_INVALID; }


int lsm_hcond_apply(LsmHcond* s, const double* x, double* y) {
    if (!s) return LSM_ERR_INVALID;
    if (!x || !y || x == y) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_apply: x and y must be two arrays");
    const HcLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, hc_apply_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, x, y);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_hcond_load(LsmHcond* s, int k, double* f_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!f_out || k < 0 || k >= s->o->K) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_load: no such unit gradient, or a null array");
    hc_launch_load(*s->o, s->h->stream, k, f_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_hcond_solve(LsmHcond* s, const double* chi_guess, double rtol, int max_iters, int* iters, double* relres) {
    if (!s) return LSM_ERR_INVALID;
    return cp_solve_all(s->h, *s->o, "lsm_hcond_solve", chi_guess, rtol, max_iters, iters, relres, [&](int k) { hc_launch_load(*s->o, s->h->stream, k, s->o->f); });
}

int lsm_hcond_solve_rhs(LsmHcond* s, const double* f, double* x, double rtol, int max_iters, int* iters, double* relres) {
    return s ? cp_solve_rhs(s->h, *s->o, "lsm_hcond_solve_rhs", f, x, rtol, max_iters, iters, relres) : LSM_ERR_INVALID;
}

int lsm_hcond_set_correctors(LsmHcond* s, const double* chi) { return s ? cp_set_correctors(s->h, *s->o, "lsm_hcond_set_correctors", chi) : LSM_ERR_INVALID; }

int lsm_hcond_correctors(LsmHcond* s, double* chi_out) { return s ? cp_correctors(s->h, *s->o, "lsm_hcond_correctors", chi_out) : LSM_ERR_INVALID; }

int lsm_hcond_energy_cells(LsmHcond* s, int p, int q, double* out) {
    if (!s) return LSM_ERR_INVALID;
    HcondObject& o = *s->o;
    if (!out || p < 0 || q < 0 || p >= o.K || q >= o.K) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_energy_cells: no such pair of unit gradients, or a null array");
    const HcLevel& L = o.lev[0];
    MG_LAUNCH(o.N, hc_energy_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, (const double*)(o.chi + (size_t)p * L.nn),
              (const double*)(o.chi + (size_t)q * L.nn), p, q, out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_hcond_tensor(LsmHcond* s, double* K) {
    if (!s) return LSM_ERR_INVALID;
    return cp_tensor(s->h, *s->o, "lsm_hcond_tensor", K, [&](int sens) { hc_launch_tensor(*s->o, s->h->stream, sens); });
}

int lsm_hcond_corrector(LsmHcond* s, int k, void* u) {
    if (!s) return LSM_ERR_INVALID;
    if (k < 0 || k >= s->o->K || !u) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_corrector: no such unit gradient, or a null field");
    return cp_store(s->h, *s->o, k, CpFields{{u, nullptr, nullptr}});
}

int lsm_hcond_sensitivity(LsmHcond* s, const double* W, void* g_out) {
    if (!s) return LSM_ERR_INVALID;
    return cp_sensitivity(s->h, *s->o, "lsm_hcond_sensitivity", W, g_out, [&](int sens) { hc_launch_tensor(*s->o, s->h->stream, sens); });
}


void lsm_hcond_destroy(LsmHcond* s) {
    if (!s) return;
    delete s->o;
    delete s;
}
