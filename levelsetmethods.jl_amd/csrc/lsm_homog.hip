// lsm_homog.hip — homogenize: the effective elasticity tensor C^H of the periodic material whose cell is the box of ϕ, and its
// sensitivity.  The Q1 operator of lsm_elastic.hip on the torus of the grid's cells (period n − 1 cells: node n − 1 is node 0), the
// M = N(N+1)/2 cell problems A χ^k = f^k solved by cell_problem.h over mg_pcg.h's conjugate gradients with a wrapping V-cycle, then
// one pass over the cells for the tensor.  DESIGN.md §7.23; include/lsm.h ("homogenize") is the normative text, tests/_homog_ref.py
// restates it.  Built with -ffp-contract=off: the cell array, A x, the loads, the cell integrands and the sensitivity round as numpy does.
//
// Storage.  cell_problem.h's, with N components per node and M correctors of N·nn doubles.
//
// What is mg_pcg.h's: the state, K2, the smoother, the coarsest kernel, the V-cycle's driver, the iteration loop, the report.  What is
// cell_problem.h's: the wrapped index arithmetic and transfers, the Level's base, the hierarchy, the allocation, the setup and its
// refusals, the PCG's start, init, direction and K1 kernels, the solves, the correctors' storage, the host tails of the tensor and
// the sensitivity, its gather, the store.  What is this file's own: K0 per level, the wrapping apply (the Level), the diagonal, the
// load, χ0 and g, and the cell kernels.
#include <memory>

#include "cell_problem.h"
#include "el_k0.h"

namespace lsm {

static const double HG_OMEGA = 0.6, HG_SAFE = 1.9;      // lsm_elastic.hip's damping rule

struct HgLevel : CpLevel<HgLevel> {
    int n[3];                     // nodes (= cells) of the torus per axis
    int nn;
    double h[3];
    const double* cell;           // cell moduli
    const double* D;              // the diagonal, component-major
    const double* K;              // the level's K0, (2^N·N)² row-major
    double om;                    // min(HG_OMEGA, HG_SAFE/λ)

    static constexpr int comps(int N) { return N; }
    __device__ __forceinline__ bool fixed(int id, int) const { return id == 0; }
    __device__ __forceinline__ double omega() const { return om; }
    // the operator's N rows at a node; x holds zero at node 0, so there is nothing to mask
    template <int N, bool MASK>
    __device__ __forceinline__ void apply(int id, const int I[3], const double* x, int stride, double out[N]) const;
};

// (A x)_{I,·} in lsm_elastic.hip's order: the 2^N cells around I ascending (bit d of m set: cell I_d, clear: cell I_d − 1, wrapped);
// per cell and row the columns from +0, corner b ascending, component j fastest; then the cell's modulus; the cell terms from +0.
// xat(q, j): component j at node q.
template <int N, class X>
__device__ __forceinline__ void hg_apply(const HgLevel& L, const int I[3], X xat, double out[N]) {
    constexpr int NC = 1 << N, NB = N == 2 ? 9 : 27, R = NC * N;
    int c[3][3];
    mg_wrapped<N>(L.n, I, c);
    double v[NB][N];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int q = c[0][k % 3] + c[1][(k / 3) % 3] + (N > 2 ? c[2][k / 9] : 0);
#pragma unroll
        for (int j = 0; j < N; ++j) v[k][j] = xat(q, j);
    }
    const double* __restrict__ K = L.K;
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = 0.0;
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        const double E = L.cell[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
        const int a = (~m) & (NC - 1);
        double inner[N];
#pragma unroll
        for (int i = 0; i < N; ++i) inner[i] = 0.0;
#pragma unroll
        for (int b = 0; b < NC; ++b) {
            const int o0 = (m & 1) + (b & 1), o1 = ((m >> 1) & 1) + ((b >> 1) & 1), o2 = N > 2 ? ((m >> 2) & 1) + ((b >> 2) & 1) : 0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double val = v[o0 + 3 * o1 + (N > 2 ? 9 * o2 : 0)][j];
#pragma unroll
                for (int i = 0; i < N; ++i) inner[i] = inner[i] + K[(a * N + i) * R + b * N + j] * val;
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) out[i] = out[i] + E * inner[i];
    }
}

template <int N, bool MASK>
__device__ __forceinline__ void HgLevel::apply(int id, const int I[3], const double* x, int stride, double out[N]) const {
    hg_apply<N>(*this, I, [&](int q, int j) { return x[j * stride + q]; }, out);
}

// ---- the diagonal: D_{I,i} = Σ_C E_C·K0[(a,i),(a,i)], the cells ascending, from +0
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_diag_kernel(HgLevel L, double* __restrict__ D) {
    constexpr int NC = 1 << N, R = NC * N;
    MG_LOOP(id, L.nn) {
        int I[3], c[3][3];
        mg_coords<N>(L.n, id, I);
        mg_wrapped<N>(L.n, I, c);
        double acc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = 0.0;
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const double E = L.cell[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
            const int a = (~m) & (NC - 1);
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] = acc[i] + E * L.K[(a * N + i) * R + a * N + i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) D[i * L.nn + id] = acc[i];
    }
}

// ---- the load of unit strain k: f_{I,i} = −Σ_C E_C·g[(a,i)], the cells ascending, from +0; g = K0·χ0^k (2^N·N doubles)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_load_kernel(HgLevel L, const double* __restrict__ g, double* __restrict__ f) {
    constexpr int NC = 1 << N;
    MG_LOOP(id, L.nn) {
        int I[3], c[3][3];
        mg_coords<N>(L.n, id, I);
        mg_wrapped<N>(L.n, I, c);
        double acc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = 0.0;
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const double E = L.cell[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
            const int a = (~m) & (NC - 1);
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] = acc[i] + E * g[a * N + i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) f[i * L.nn + id] = -acc[i];
    }
}

// ---- y = A x on all components, no pin (lsm_homog_apply)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_apply_kernel(HgLevel L, const double* __restrict__ x, double* __restrict__ y) {
    const int nn = L.nn;
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double out[N];
        hg_apply<N>(L, I, [&](int q, int j) { return x[j * nn + q]; }, out);
#pragma unroll
        for (int i = 0; i < N; ++i) y[i * nn + id] = out[i];
    }
}

// ---- the cell kernels.  w^k = χ0^k + χ^k at a cell's 2^N·N corner values; t^{pq}_C = E_C·(Σ_r w^p_r·(Σ_s K0[r,s]·w^q_s)), both from +0
// t^{pq} of every cell, for one pair (lsm_homog_energy_cells)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_energy_kernel(HgLevel L, const double* __restrict__ chip, const double* __restrict__ chiq,
                                                               const double* __restrict__ c0p, const double* __restrict__ c0q, double* __restrict__ out) {
    constexpr int NC = 1 << N, R = NC * N;
    const double* __restrict__ K = L.K;
    const int nn = L.nn;
    MG_LOOP(id, nn) {
        int C[3], node[NC];
        mg_coords<N>(L.n, id, C);
        mg_wrapped_corners<N>(L.n, C, node);
        double wp[R], wq[R];
#pragma unroll
        for (int b = 0; b < NC; ++b)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                wp[b * N + j] = c0p[b * N + j] + chip[j * nn + node[b]];
                wq[b * N + j] = c0q[b * N + j] + chiq[j * nn + node[b]];
            }
        double d = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double t = 0.0;
#pragma unroll
            for (int s = 0; s < R; ++s) t = t + K[r * R + s] * wq[s];
            d = d + wp[r] * t;
        }
        out[id] = L.cell[id] * d;
    }
}

// all M(M+1)/2 sums Σ_C t^{pq}_C, p ≤ q, in one pass: K0·w^q once per q, dotted with w^p for p ≤ q; entry e counts q ascending, within it
// p ascending.  A thread holds the M·2^N·N corner values of its cell (144 doubles in 3-D) and one K0·w^q: no scratch at 256 threads.
// SENS (lsm_homog_sensitivity): no reduction; the same pairs in the same order, cell[C] = Σ_q Σ_{p ≤ q} c·W[p·M + q]·t^{pq}_C from +0, c = 2
// for p < q (W is symmetric, and t^{qp} is t^{pq} as in the mirrored tensor): w^p for p > q is not needed, so the corner values
// are loaded as q advances and the 3-D kernel stays without scratch.
template <int N, int SENS>
__global__ void __launch_bounds__(MG_THREADS) hg_tensor_kernel(HgLevel L, const double* __restrict__ chi, const double* __restrict__ chi0,
                                                               const double* __restrict__ W, double* __restrict__ cell, double* partial, unsigned* ticket,
                                                               double* __restrict__ out) {
    constexpr int NC = 1 << N, R = NC * N, M = N * (N + 1) / 2, NP = M * (M + 1) / 2;
    const double* __restrict__ K = L.K;
    const int nn = L.nn;
    const size_t nt = (size_t)N * nn;
    double red[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) red[e] = 0.0;
    MG_LOOP(id, nn) {
        int C[3], node[NC];
        mg_coords<N>(L.n, id, C);
        mg_wrapped_corners<N>(L.n, C, node);
        const double E = L.cell[id];
        double w[M][R];
#pragma unroll
        for (int k = 0; k < M; ++k)
#pragma unroll
            for (int b = 0; b < NC; ++b)
#pragma unroll
                for (int j = 0; j < N; ++j) w[k][b * N + j] = chi0[k * R + b * N + j] + chi[k * nt + (size_t)j * nn + node[b]];
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < M; ++q) {
            double kw[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double t = 0.0;
#pragma unroll
                for (int s = 0; s < R; ++s) t = t + K[r * R + s] * w[q][s];
                kw[r] = t;
            }
#pragma unroll
            for (int p = 0; p <= q; ++p) {
                double d = 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r) d = d + w[p][r] * kw[r];
                if (SENS) acc = acc + (p < q ? 2.0 * W[p * M + q] : W[p * M + q]) * (E * d);
                else red[q * (q + 1) / 2 + p] += E * d;
            }
        }
        if (SENS) cell[id] = acc;
    }
    if (SENS) return;
    if (!block_reduce_ordered<NP, MG_THREADS>(red, partial, ticket) || threadIdx.x != 0) return;
#pragma unroll
    for (int e = 0; e < NP; ++e) out[e] = red[e];
}

// ---- host side
struct HomogObject : CellProblem<HgLevel> {
    std::vector<std::vector<double>> k0;     // the levels' K0 as computed (what the device holds)
    double *chi0 = nullptr, *g = nullptr;    // χ0^k at a cell's corners and g^k = K0·χ0^k, of every unit strain
};

// the Voigt pairs in the header's order
static void hg_voigt(int N, int k, int& i, int& j) {
    static const int v2[3][2] = {{0, 0}, {1, 1}, {0, 1}}, v3[6][2] = {{0, 0}, {1, 1}, {2, 2}, {1, 2}, {0, 2}, {0, 1}};
    i = N == 2 ? v2[k][0] : v3[k][0];
    j = N == 2 ? v2[k][1] : v3[k][1];
}

static void hg_launch_load(HomogObject& o, hipStream_t st, int k, double* f) {
    const HgLevel& L = o.lev[0];
    MG_LAUNCH(o.N, hg_load_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, (const double*)(o.g + (size_t)k * (1 << o.N) * o.N), f);
}
// the tensor kernel: sens = 0 leaves the sums in o.sums, sens = 1 reads o.W and leaves a value per cell in o.cell
static void hg_launch_tensor(HomogObject& o, hipStream_t st, int sens) {
    const HgLevel& L = o.lev[0];
    const unsigned nb = mg_blocks(L.nn);
    unsigned* ticket = &o.st.p->ticket[3];
    if (sens) MG_LAUNCH2(o.N, hg_tensor_kernel, 1, dim3(nb), MG_THREADS, st, L, (const double*)o.chi, (const double*)o.chi0, (const double*)o.W, o.cell, o.tpartial.p, ticket, o.sums);
    else MG_LAUNCH2(o.N, hg_tensor_kernel, 0, dim3(nb), MG_THREADS, st, L, (const double*)o.chi, (const double*)o.chi0, (const double*)o.W, o.cell, o.tpartial.p, ticket, o.sums);
}

}  // namespace lsm

using namespace lsm;

struct LsmHomog { LsmHandle* h; HomogObject* o; };

static int hg_create(LsmHandle* h, HomogObject& o, const void* phi, double level, double e_in, double e_out, const double* e_cells, double lam, double mu,
                     int64_t stats[4]) {
    std::vector<HgLevel> lev;
    double hmin;
    cp_shapes(h, o, 1LL << 28, lev, hmin);
    if (lev.empty()) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: the grid is too large (2^28 nodes at most)");
    const int N = o.N, nl = (int)lev.size(), M = o.K = N * (N + 1) / 2, R = (1 << N) * N;
    const size_t RR = (size_t)R * R;
    // the operator's own doubles: per level K0; at the end χ0 and g of every unit strain
    CpCarve c;
    const int ra = cp_alloc(h, o, lev, RR, 2 * (size_t)M * R, c);
    if (ra != LSM_OK) return ra;
    hipStream_t s = h->stream;
    o.k0.resize(nl);
    for (int l = 0; l < nl; ++l) {
        lev[l].K = c.own[l];
        es_k0(N, lev[l].h, lam, mu, o.k0[l]);
        lev[l].om = std::min(HG_OMEGA, HG_SAFE / es_symbol_lambda(N, o.k0[l]));
        LSM_HIP(h, hipMemcpyAsync(c.own[l], o.k0[l].data(), RR * sizeof(double), hipMemcpyHostToDevice, s));
    }
    o.chi0 = c.own[nl];
    o.g = o.chi0 + (size_t)M * R;
    // χ0^k at a cell's corners (corner a at x_d = bit_d(a)·h_d) and g^k = K0·χ0^k, the row's sum from +0 ascending
    std::vector<double> c0((size_t)M * R, 0.0), g((size_t)M * R, 0.0);
    for (int k = 0; k < M; ++k) {
        int i, j;
        hg_voigt(N, k, i, j);
        for (int a = 0; a < (1 << N); ++a) {
            const double xi = ((a >> i) & 1) * lev[0].h[i], xj = ((a >> j) & 1) * lev[0].h[j];
            if (i == j) c0[(size_t)k * R + a * N + i] = xi;
            else {
                c0[(size_t)k * R + a * N + i] = 0.5 * xj;
                c0[(size_t)k * R + a * N + j] = 0.5 * xi;
            }
        }
        for (int r = 0; r < R; ++r) {
            double t = 0.0;
            for (int q = 0; q < R; ++q) t = t + o.k0[0][(size_t)r * R + q] * c0[(size_t)k * R + q];
            g[(size_t)k * R + r] = t;
        }
    }
    LSM_HIP(h, hipMemcpyAsync(o.chi0, c0.data(), c0.size() * sizeof(double), hipMemcpyHostToDevice, s));
    LSM_HIP(h, hipMemcpyAsync(o.g, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, s));
    return cp_setup(h, o, lev, c, "lsm_homog_create", "moduli", phi, level, e_in, e_out, e_cells, hmin, stats,
                    [&](const HgLevel& Ll, double* D) { MG_LAUNCH(N, hg_diag_kernel, dim3(mg_blocks(Ll.nn)), MG_THREADS, s, Ll, D); });
}

int lsm_homog_create(LsmHandle* h, const void* phi, double level, double e_in, double e_out, const double* e_cells, double nu, int plane, int precond,
                     LsmHomog** out, int64_t stats[4]) {
    const int rc = cp_create_check(h, out, stats, "lsm_homog_create", "moduli", "e_in", "e_out", phi, e_cells, level, e_in, e_out);
    if (rc != LSM_OK) return rc;
    if (!std::isfinite(nu) || !(nu > -1.0) || !(nu < 0.5)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: nu must be finite with -1 < nu < 0.5");
    if (plane != LSM_PLANE_STRESS && plane != LSM_PLANE_STRAIN) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: unknown plane (LSM_PLANE_STRESS or LSM_PLANE_STRAIN)");
    const int rp = cp_check_precond(h, "lsm_homog_create", precond);
    if (rp != LSM_OK) return rp;
    const int N = h->grid.ndim;
    const double mu = 1.0 / (2.0 * (1.0 + nu));
    const double lam = (N == 2 && plane == LSM_PLANE_STRESS) ? nu / (1.0 - nu * nu) : nu / ((1.0 + nu) * (1.0 - 2.0 * nu));
    (void)hipSetDevice(h->device);
    std::unique_ptr<HomogObject> o(new HomogObject());
    o->precond = precond;
    const int r = hg_create(h, *o, phi, level, e_in, e_out, e_cells, lam, mu, stats);
    if (r != LSM_OK) return r;
    *out = new LsmHomog{h, o.release()};
    return LSM_OK;
}

int lsm_homog_stiffness(LsmHomog* s, int level, double* k0_host) {
    if (!s) return LSM_ERR_INVALID;
    if (!k0_host || level < 0 || level >= (int)s->o->k0.size()) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_stiffness: no such level, or a null array");
    memcpy(k0_host, s->o->k0[level].data(), s->o->k0[level].size() * sizeof(double));
    return LSM_OK;
}

int lsm_homog_cells(LsmHomog* s, double* e_out_cells) { return s ? cp_cells(s->h, *s->o, "lsm_homog_cells", e_out_cells) : LSM_ERR_INVALID; }

int lsm_homog_apply(LsmHomog* s, const double* x, double* y) {
    if (!s) return LSM_ERR_INVALID;
    if (!x || !y || x == y) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_apply: x and y must be two arrays");
    const HgLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, hg_apply_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, x, y);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_homog_load(LsmHomog* s, int k, double* f_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!f_out || k < 0 || k >= s->o->K) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_load: no such unit strain, or a null array");
    hg_launch_load(*s->o, s->h->stream, k, f_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_homog_solve(LsmHomog* s, const double* chi_guess, double rtol, int max_iters, int* iters, double* relres) {
    if (!s) return LSM_ERR_INVALID;
    return cp_solve_all(s->h, *s->o, "lsm_homog_solve", chi_guess, rtol, max_iters, iters, relres, [&](int k) { hg_launch_load(*s->o, s->h->stream, k, s->o->f); });
}

int lsm_homog_solve_rhs(LsmHomog* s, const double* f, double* x, double rtol, int max_iters, int* iters, double* relres) {
    return s ? cp_solve_rhs(s->h, *s->o, "lsm_homog_solve_rhs", f, x, rtol, max_iters, iters, relres) : LSM_ERR_INVALID;
}

int lsm_homog_set_correctors(LsmHomog* s, const double* chi) { return s ? cp_set_correctors(s->h, *s->o, "lsm_homog_set_correctors", chi) : LSM_ERR_INVALID; }

int lsm_homog_correctors(LsmHomog* s, double* chi_out) { return s ? cp_correctors(s->h, *s->o, "lsm_homog_correctors", chi_out) : LSM_ERR_INVALID; }

int lsm_homog_energy_cells(LsmHomog* s, int p, int q, double* out) {
    if (!s) return LSM_ERR_INVALID;
    HomogObject& o = *s->o;
    if (!out || p < 0 || q < 0 || p >= o.K || q >= o.K) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_energy_cells: no such pair of unit strains, or a null array");
    const HgLevel& L = o.lev[0];
    const size_t nt = o.nt(), R = (size_t)(1 << o.N) * o.N;
    MG_LAUNCH(o.N, hg_energy_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, (const double*)(o.chi + p * nt), (const double*)(o.chi + q * nt),
              (const double*)(o.chi0 + p * R), (const double*)(o.chi0 + q * R), out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_homog_tensor(LsmHomog* s, double* C) {
    if (!s) return LSM_ERR_INVALID;
    return cp_tensor(s->h, *s->o, "lsm_homog_tensor", C, [&](int sens) { hg_launch_tensor(*s->o, s->h->stream, sens); });
}

int lsm_homog_corrector(LsmHomog* s, int k, void* u0, void* u1, void* u2) {
    if (!s) return LSM_ERR_INVALID;
    HomogObject& o = *s->o;
    CpFields U;
    U.p[0] = u0; U.p[1] = u1; U.p[2] = o.N > 2 ? u2 : nullptr;
    if (k < 0 || k >= o.K || !u0 || !u1 || u0 == u1 || (o.N > 2 && (!u2 || u2 == u0 || u2 == u1)))
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_corrector: no such unit strain, or the N fields are not distinct");
    return cp_store(s->h, o, k, U);
}

int lsm_homog_sensitivity(LsmHomog* s, const double* W, void* g_out) {
    if (!s) return LSM_ERR_INVALID;
    return cp_sensitivity(s->h, *s->o, "lsm_homog_sensitivity", W, g_out, [&](int sens) { hg_launch_tensor(*s->o, s->h->stream, sens); });
}

void lsm_homog_destroy(LsmHomog* s) {
    if (!s) return;
    delete s->o;
    delete s;
}
