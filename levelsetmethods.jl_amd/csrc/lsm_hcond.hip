// lsm_hcond.hip — homogenize_conductivity: the effective conductivity tensor K^H of −∇·(a∇u) for the periodic material whose cell is
// the box of ϕ, and its sensitivity.  lsm_elliptic.hip's edge operator with c = 0 on the torus of the grid's cells (period n − 1
// cells: node n − 1 is node 0), the N cell problems A χ^p = f^p solved by mg_pcg.h's conjugate gradients with a wrapping V-cycle, then
// one pass over the cells for the tensor.  DESIGN.md §7.24; include/lsm.h ("homogenize_conductivity") is the normative text,
// tests/_hcond_ref.py restates it.  Built with -ffp-contract=off: the cell array, A x, the loads, the cell integrands and the
// sensitivity round as numpy does.
//
// Storage.  lsm_homog.hip's: a level has m nodes per axis and as many cells, node I and cell I (lowest corner I) share the linear
// index I0 + m0·(I1 + m1·I2).  Solver vectors are fp64, one component.  Node 0 is pinned to zero on every level, which removes the
// constants.  The correctors are kept on the device, N vectors of nn doubles; a solve writes them only when all N have converged.
//
// What is mg_pcg.h's: the state, K2, the smoother, the coarsest kernel, the wrapping transfers, the V-cycle's driver, the iteration
// loop, the report, the wrapped index arithmetic.  What is this file's own: the wrapping edge operator (the Level), the load, and the cell
// kernels.
#include <memory>

#include "el_cell.h"
#include "mg_pcg.h"

namespace lsm {

static const double HC_OMEGA = 0.8;      // lsm_elliptic.hip's damping
enum { HC_BAD_PHI = 0, HC_BAD_A = 1, HC_NSTAT = 4 };
static const int HC_MAXP = 6;            // N(N+1)/2 in 3-D

struct HcVec : MgVec { double* p; };     // the search direction, updated in place
struct HcShape { int n[3]; };            // the handle's dense grid (nodes)

struct HcLevel {
    int n[3];                     // nodes (= cells) of the torus per axis
    int nn;
    double h[3], ih2[3];
    const double* a;              // cell coefficients
    const double* D;              // the diagonal

    using Vec = HcVec;
    static constexpr bool wraps = true;
    static constexpr int comps(int) { return 1; }
    __device__ __forceinline__ bool fixed(int id, int) const { return id == 0; }
    __device__ __forceinline__ static double omega() { return HC_OMEGA; }
    static void launch_resid(int N, unsigned nb, hipStream_t s, const HcLevel& L, const double* r, const double* x, double* res, const MgState* st);
    static void launch_gather(int N, hipStream_t s, const HcLevel& Lf, const HcLevel& Lc, const int co[3], const double* res, double* rc, const MgState* st);
    static void launch_prolong(int N, hipStream_t s, const HcLevel& Lf, const HcLevel& Lc, const int co[3], const double* xc, double* x, const MgState* st);
    // the operator's row at a node; x holds zero at node 0, so there is nothing to mask
    template <int N, bool MASK>
    __device__ __forceinline__ void apply(int id, const int I[3], const double* x, int stride, double out[1]) const;
};

// the 2^N cells around node I: bit d of m set: cell I_d along d, clear: cell I_d − 1, wrapped
template <int N>
__device__ __forceinline__ void hc_cells_around(const HcLevel& L, const int c[3][3], double v[1 << N]) {
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) v[m] = L.a[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
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

// ---- setup of level 0: ϕ checked at every node of the dense grid; the cell coefficients from ϕ (el_cell.h: lsm_elliptic's array, the
// same bits) or the caller's, checked
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_setup_kernel(HcShape G, MgField F, const void* __restrict__ phi, double level, double a_in, double a_out,
                                                              double hmin, const double* __restrict__ a_given, double* __restrict__ a, unsigned long long* st) {
    unsigned cnt[2] = {0, 0};
    const int nnf = G.n[0] * G.n[1] * G.n[2];
    MG_LOOP(id, nnf) {
        int I[3];
        mg_coords<N>(G.n, id, I);
        if (phi && !mg_finite(ld_val(phi, mg_padded(F, I), F.f32))) ++cnt[HC_BAD_PHI];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && I[d] < G.n[d] - 1;
        if (!corner) continue;
        const int ci = mg_cell_index<N>(G.n, I);
        double av;
        if (a_given) {
            av = a_given[ci];
            if (!(av > 0.0) || !mg_finite(av)) ++cnt[HC_BAD_A];
        } else {
            av = el_cell_from_phi<N>(phi, mg_padded(F, I), F.s1, F.s2, F.f32, level, a_in, a_out, hmin);
            if (!(av > 0.0)) ++cnt[HC_BAD_A];
        }
        a[ci] = av;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned v = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&st[k], (unsigned long long)v);
    }
}

// ---- a coarse level's cells: mg_cell_average of the cells {2J, 2J+1} per coarsened axis (a level with m cells per axis is
// mg_cell_index's grid of m + 1 nodes)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_coarsen_kernel(HcLevel Lf, HcLevel Lc, int co0, int co1, int co2, double* __restrict__ ac) {
    const int co[3] = {co0, co1, co2};
    const int nf[3] = {Lf.n[0] + 1, Lf.n[1] + 1, Lf.n[2] + 1};
    const double scale = mg_coarsen_scale(co0 + co1 + co2);
    MG_LOOP(id, Lc.nn) {
        int J[3];
        mg_coords<N>(Lc.n, id, J);
        ac[id] = mg_cell_average<N>(Lf.a, nf, J, co, scale);
    }
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

// ---- PCG
// x₀ = the guess (zero without one) with the pin at zero, p = 0
__global__ void __launch_bounds__(MG_THREADS) hc_start_kernel(int nn, const double* __restrict__ guess, double* __restrict__ x, double* __restrict__ p) {
    MG_LOOP(t, nn) {
        x[t] = (guess && t != 0) ? guess[t] : 0.0;
        p[t] = 0.0;
    }
}
// r₀ = f − A x₀ away from the pin, 0 there; ‖f_free‖², ‖r₀‖²; jac: z = r/D and ρ = r·z as well
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_init_kernel(HcLevel L, HcVec V, const double* __restrict__ x, const double* __restrict__ f,
                                                             double* __restrict__ rv, double* __restrict__ zv, int jac) {
    double red[4] = {0.0, 0.0, 0.0, 0.0};
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const double ui = x[id], fi = f[id];
        if (!mg_finite(ui) || !mg_finite(fi)) red[3] += 1.0;
        double r = 0.0, z = 0.0;
        if (id != 0) {
            r = fi - hc_apply<N>(L, I, ui, [&](int q) { return x[q]; });
            red[0] += fi * fi;
            red[1] += r * r;
            if (jac) {
                z = r / L.D[id];
                red[2] += r * z;
            }
        }
        rv[id] = r;
        if (jac) zv[id] = z;
    }
    if (!block_reduce_ordered<4, MG_THREADS>(red, V.partial, &V.st->ticket[0]) || threadIdx.x != 0) return;
    mg_init_tail(*V.st, red, jac);
}
// p = z + β p, in place (both are zero at the pin)
__global__ void __launch_bounds__(MG_THREADS) hc_dir_kernel(int nn, HcVec V) {
    if (V.st->status != MG_RUN) return;
    const double beta = V.st->beta;
    const double* __restrict__ z = V.z;
    double* __restrict__ p = V.p;
    MG_LOOP(k, nn) p[k] = z[k] + beta * p[k];
}
// K1: q = A p, σ = p·q, α = ρ/σ
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_k1_kernel(HcLevel L, const double* __restrict__ p, double* __restrict__ qv, double* partial, MgState* st) {
    if (st->status != MG_RUN) return;
    double red[1] = {0.0};
    MG_LOOP(id, L.nn) {
        double q = 0.0;
        if (id != 0) {
            int I[3];
            mg_coords<N>(L.n, id, I);
            const double pi = p[id];
            q = hc_apply<N>(L, I, pi, [&](int j) { return p[j]; });
            red[0] += pi * q;
        }
        qv[id] = q;
    }
    if (!block_reduce_ordered<1, MG_THREADS>(red, partial, &st->ticket[1]) || threadIdx.x != 0) return;
    mg_k1_tail(*st, red[0]);
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
        out[id] = hc_pair<N>(L.a[id], gp, gq);
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
        const double ac = L.a[id];
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

// s_I = (Σ_C around I of cell[C], ascending, from +0)·2^−N at every node of the handle's grid (node n − 1 is node 0), rounded once
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_sens_gather_kernel(HcLevel L, HcShape G, MgField F, const double* __restrict__ cell, void* __restrict__ g_out) {
    const int nnf = G.n[0] * G.n[1] * G.n[2];
    MG_LOOP(id, nnf) {
        int I[3], T[3] = {0, 0, 0}, c[3][3];
        mg_coords<N>(G.n, id, I);
#pragma unroll
        for (int d = 0; d < N; ++d) T[d] = I[d] == L.n[d] ? 0 : I[d];
        mg_wrapped<N>(L.n, T, c);
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < (1 << N); ++m) acc = acc + cell[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
        st_val(g_out, mg_padded(F, I), F.f32, acc * (N == 2 ? 0.25 : 0.125));
    }
}

// χ^p into a field of the handle, the image nodes n − 1 from node 0, rounded once
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hc_store_kernel(HcLevel L, HcShape G, MgField F, const double* __restrict__ x, void* __restrict__ u) {
    const int nnf = G.n[0] * G.n[1] * G.n[2];
    MG_LOOP(id, nnf) {
        int I[3], T[3] = {0, 0, 0};
        mg_coords<N>(G.n, id, I);
#pragma unroll
        for (int d = 0; d < N; ++d) T[d] = I[d] == L.n[d] ? 0 : I[d];
        st_val(u, mg_padded(F, I), F.f32, x[T[0] + L.n[0] * (T[1] + (N > 2 ? L.n[1] * T[2] : 0))]);
    }
}

// ---- host side
void HcLevel::launch_resid(int N, unsigned nb, hipStream_t s, const HcLevel& L, const double* r, const double* x, double* res, const MgState* st) {
    MG_LAUNCH2(N, mg_resid_kernel, HcLevel, dim3(nb), dim3(MG_THREADS), s, L, r, x, res, st);
}
void HcLevel::launch_gather(int N, hipStream_t s, const HcLevel& Lf, const HcLevel& Lc, const int co[3], const double* res, double* rc, const MgState* st) {
    MG_LAUNCH2(N, mg_wrap_gather_kernel, HcLevel, dim3(mg_blocks(Lc.nn), 1), MG_THREADS, s, Lf, Lc, co[0], co[1], co[2], res, rc, st);
}
void HcLevel::launch_prolong(int N, hipStream_t s, const HcLevel& Lf, const HcLevel& Lc, const int co[3], const double* xc, double* x, const MgState* st) {
    MG_LAUNCH2(N, mg_wrap_prolong_kernel, HcLevel, dim3(mg_blocks(Lf.nn), 1), MG_THREADS, s, Lf, Lc, co[0], co[1], co[2], xc, x, st);
}

struct HcondObject : MgSolver<HcLevel> {
    HcShape G;                               // the handle's dense grid
    double *chi = nullptr, *chinew = nullptr, *f = nullptr, *cell = nullptr, *W = nullptr, *sums = nullptr;
    DevBuf<double> tpartial;                 // the tensor kernel's partials: HC_MAXP per workgroup
    PinnedBuf<double> h_sums;
};

}  // namespace lsm

using namespace lsm;

struct LsmHcond { LsmHandle* h; HcondObject* o; };

static int hc_create(LsmHandle* h, HcondObject& o, const void* phi, double level, double a_in, double a_out, const double* a_cells, int64_t stats[4]) {
    const int N = h->grid.ndim;
    o.N = N;
    o.F = MgField{h->lay.stride[1], N > 2 ? h->lay.stride[2] : 0, h->lay.origin, h->dtype == LSM_DTYPE_F32 ? 1 : 0};
    // the hierarchy: axis d coarsens while m_d is even and above 4
    std::vector<HcLevel> lev;
    HcLevel L;
    memset(&L, 0, sizeof(L));
    long long nn = 1, nnf = 1;
    double hmin = INFINITY;
    for (int d = 0; d < 3; ++d) {
        o.G.n[d] = d < N ? h->nloc[d] : 1;
        L.n[d] = d < N ? h->nloc[d] - 1 : 1;
        L.h[d] = d < N ? h->h[d] : 1.0;
        nn *= L.n[d];
        nnf *= o.G.n[d];
        if (d < N) hmin = std::min(hmin, L.h[d]);
    }
    if (nnf >= (1LL << 29)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: the grid is too large (2^29 nodes at most)");
    L.nn = (int)nn;
    lev.push_back(L);
    for (;;) {
        const HcLevel& f = lev.back();
        HcLevel c = f;
        bool any = false;
        const int l = (int)lev.size() - 1;
        c.nn = 1;
        for (int d = 0; d < 3; ++d) {
            o.co[l][d] = d < N && f.n[d] % 2 == 0 && f.n[d] > 4;
            if (o.co[l][d]) {
                any = true;
                c.n[d] = f.n[d] / 2;
                c.h[d] = f.h[d] * 2.0;
            }
            c.nn *= c.n[d];
        }
        if (!any || lev.size() >= 31) break;
        lev.push_back(c);
    }
    for (HcLevel& q : lev)
        for (int d = 0; d < 3; ++d) q.ih2[d] = 1.0 / (q.h[d] * q.h[d]);
    const int nl = (int)lev.size();
    // one allocation of doubles: per level cells, D, xa, xb, [rhs]; level 0: x r q p, f, the cell scratch, χ and its staging copy, W, the
    // tensor's sums
    size_t nd = 0;
    for (int l = 0; l < nl; ++l) nd += (size_t)lev[l].nn * (size_t)(4 + (l ? 1 : 4));
    nd += 2 * (size_t)nn + 2 * (size_t)N * (size_t)nn + (size_t)N * N + HC_MAXP;
    LSM_HIP(h, o.buf.alloc(nd * sizeof(double)));
    LSM_HIP(h, o.tpartial.alloc((size_t)HC_MAXP * MG_MAXB * sizeof(double)));
    LSM_HIP(h, o.h_sums.alloc(HC_MAXP * sizeof(double)));
    hipStream_t s = h->stream;
    const int ra = mg_alloc_scalars(h, o, HC_NSTAT, s);
    if (ra != LSM_OK) return ra;
    double* b = o.buf;
    std::vector<double*> acell(nl), dg(nl);
    o.rhs.assign(nl, nullptr); o.xa.assign(nl, nullptr); o.xb.assign(nl, nullptr);
    for (int l = 0; l < nl; ++l) {
        const size_t m = (size_t)lev[l].nn;
        acell[l] = b; b += m;
        dg[l] = b; b += m;
        o.xa[l] = b; b += m;
        o.xb[l] = b; b += m;
        if (l) { o.rhs[l] = b; b += m; }
        else {
            o.V.x = b; b += m; o.V.r = b; b += m; o.V.q = b; b += m; o.V.p = b; b += m;
        }
        lev[l].a = acell[l]; lev[l].D = dg[l];
    }
    o.f = b; b += nn;
    o.cell = b; b += nn;
    o.chi = b; b += (size_t)N * nn;
    o.chinew = b; b += (size_t)N * nn;
    o.W = b; b += (size_t)N * N;
    o.sums = b; b += HC_MAXP;
    LSM_HIP(h, hipMemsetAsync(o.chi, 0, (size_t)N * nn * sizeof(double), s));
    MG_LAUNCH(N, hc_setup_kernel, dim3(mg_blocks(nnf)), MG_THREADS, s, o.G, o.F, a_cells ? (const void*)nullptr : phi, level, a_in, a_out, hmin, a_cells, acell[0],
              o.cnt.p);
    LSM_HIP(h, hipGetLastError());
    unsigned long long c[HC_NSTAT] = {};
    LSM_HIP(h, hipMemcpyAsync(c, o.cnt.p, sizeof(c), hipMemcpyDeviceToHost, s));
    LSM_HIP(h, hipStreamSynchronize(s));
    const int reason = c[HC_BAD_PHI] ? 1 : c[HC_BAD_A] ? 2 : 0;
    if (reason) {
        if (stats) { stats[0] = -reason; stats[1] = (int64_t)(reason == 1 ? c[HC_BAD_PHI] : c[HC_BAD_A]); stats[2] = stats[3] = 0; }
        return lsm_fail(h, LSM_ERR_INVALID, reason == 1 ? "lsm_hcond_create: phi must be finite" : "lsm_hcond_create: the cell coefficients must be finite and positive");
    }
    for (int l = 1; l < nl; ++l)
        MG_LAUNCH(N, hc_coarsen_kernel, dim3(mg_blocks(lev[l].nn)), MG_THREADS, s, lev[l - 1], lev[l], o.co[l - 1][0], o.co[l - 1][1], o.co[l - 1][2], acell[l]);
    for (int l = 0; l < nl; ++l) MG_LAUNCH(N, hc_diag_kernel, dim3(mg_blocks(lev[l].nn)), MG_THREADS, s, lev[l], dg[l]);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(s));
    o.lev = lev;
    o.nfixed = 1;
    o.nfree = nn - 1;
    o.V.z = o.precond == LSM_PRECOND_JACOBI ? o.xa[0] : o.xb[0];
    if (stats) { stats[0] = nl; stats[1] = o.nfree; stats[2] = nn; stats[3] = 0; }
    return LSM_OK;
}

int lsm_hcond_create(LsmHandle* h, const void* phi, double level, double a_in, double a_out, const double* a_cells, int precond, LsmHcond** out,
                     int64_t stats[4]) {
    if (!h || !out) return h ? lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: null argument") : LSM_ERR_INVALID;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (!phi && !a_cells) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: give phi or the cell coefficients");
    const int N = h->grid.ndim;
    if (N == 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: a 1-dimensional grid is not supported (2-D and 3-D only)");
    if (h->comm) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: the handle has a communicator attached (single device only)");
    if (h->bc[N - 1][0].kind == LSM_BC_NONE || h->bc[N - 1][1].kind == LSM_BC_NONE)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: the handle is a slab of a multi-GPU grid (whole grids only)");
    for (int d = 0; d < N; ++d)
        if (h->nloc[d] < 3) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: at least 3 nodes (2 cells) per dimension");
    if (!a_cells && (!(a_in > 0) || !std::isfinite(a_in) || !(a_out > 0) || !std::isfinite(a_out)))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: a_in and a_out must be finite and positive");
    if (!a_cells && !std::isfinite(level)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: level must be finite");
    if (precond != LSM_PRECOND_MG && precond != LSM_PRECOND_JACOBI) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_create: unknown preconditioner");
    (void)hipSetDevice(h->device);
    std::unique_ptr<HcondObject> o(new HcondObject());
    o->precond = precond;
    const int r = hc_create(h, *o, phi, level, a_in, a_out, a_cells, stats);
    if (r != LSM_OK) return r;
    *out = new LsmHcond{h, o.release()};
    return LSM_OK;
}

int lsm_hcond_cells(LsmHcond* s, double* a_out_cells) {
    if (!s) return LSM_ERR_INVALID;
    if (!a_out_cells) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_cells: null argument");
    const HcLevel& L = s->o->lev[0];
    LSM_HIP(s->h, hipMemcpyAsync(a_out_cells, L.a, (size_t)L.nn * sizeof(double), hipMemcpyDeviceToDevice, s->h->stream));
    return LSM_OK;
}

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
    HcondObject& o = *s->o;
    if (!f_out || k < 0 || k >= o.N) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_load: no such unit gradient, or a null array");
    const HcLevel& L = o.lev[0];
    MG_LAUNCH(o.N, hc_load_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, k, f_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

// A x = f away from the pin by PCG from `guess` (device, nn; NULL: zero); the solution is left in o.V.x
static int hc_pcg(LsmHandle* h, HcondObject& o, const char* fn, const double* f, const double* guess, double rtol, int max_iters, int* iters, double* relres) {
    const int N = o.N;
    const HcLevel& L = o.lev[0];
    const int jac = o.precond == LSM_PRECOND_JACOBI;
    hipStream_t st = h->stream;
    const unsigned nb = mg_blocks(L.nn);
    const int r0 = mg_reset(h, o, rtol, max_iters, st);
    if (r0 != LSM_OK) return r0;
    hipLaunchKernelGGL(hc_start_kernel, dim3(nb), dim3(MG_THREADS), 0, st, L.nn, guess, o.V.x, o.V.p);
    MG_LAUNCH(N, hc_init_kernel, dim3(nb), MG_THREADS, st, L, o.V, (const double*)o.V.x, f, o.V.r, o.V.z, jac);
    LSM_HIP(h, hipGetLastError());
    const int r1 = mg_iterate(h, o, max_iters, st, [&](int) {
        if (!jac) mg_vcycle(o, o.V.r, st);
        hipLaunchKernelGGL(hc_dir_kernel, dim3(nb), dim3(MG_THREADS), 0, st, L.nn, o.V);
        MG_LAUNCH(N, hc_k1_kernel, dim3(nb), MG_THREADS, st, L, (const double*)o.V.p, o.V.q, o.partial.p, o.st.p);
        if (jac) hipLaunchKernelGGL(mg_k2_kernel<1>, dim3(nb), dim3(MG_THREADS), 0, st, L.D, L.nn, (MgVec)o.V, (const double*)o.V.p);
        else hipLaunchKernelGGL(mg_k2_kernel<0>, dim3(nb), dim3(MG_THREADS), 0, st, L.D, L.nn, (MgVec)o.V, (const double*)o.V.p);
    });
    if (r1 != LSM_OK) return r1;
    return mg_report(h, o, fn, rtol, iters, relres);
}

int lsm_hcond_solve(LsmHcond* s, const double* chi_guess, double rtol, int max_iters, int* iters, double* relres) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    HcondObject& o = *s->o;
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_solve: rtol must be positive and max_iters at least 1");
    const int N = o.N;
    const HcLevel& L = o.lev[0];
    (void)hipSetDevice(h->device);
    hipStream_t st = h->stream;
    const size_t nn = (size_t)L.nn;
    for (int k = 0; k < N; ++k) {
        if (iters) iters[k] = 0;
        if (relres) relres[k] = 0.0;
    }
    const double* guess = nullptr;
    if (chi_guess) {      // the caller's memory, host or device: staged where the new correctors will land
        LSM_HIP(h, hipMemcpyAsync(o.chinew, chi_guess, (size_t)N * nn * sizeof(double), hipMemcpyDefault, st));
        LSM_HIP(h, hipStreamSynchronize(st));
        guess = o.chinew;
    }
    for (int k = 0; k < N; ++k) {
        MG_LAUNCH(N, hc_load_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, k, o.f);
        const int r = hc_pcg(h, o, "lsm_hcond_solve", o.f, guess ? guess + k * nn : nullptr, rtol, max_iters, iters ? iters + k : nullptr, relres ? relres + k : nullptr);
        if (r != LSM_OK) return r;      // the stored correctors are untouched
        LSM_HIP(h, hipMemcpyAsync(o.chinew + k * nn, o.V.x, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    LSM_HIP(h, hipMemcpyAsync(o.chi, o.chinew, (size_t)N * nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    LSM_HIP(h, hipStreamSynchronize(st));
    return LSM_OK;
}

int lsm_hcond_solve_rhs(LsmHcond* s, const double* f, double* x, double rtol, int max_iters, int* iters, double* relres) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    HcondObject& o = *s->o;
    if (!f || !x || f == x) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_solve_rhs: f and x must be two arrays");
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_hcond_solve_rhs: rtol must be positive and max_iters at least 1");
    (void)hipSetDevice(h->device);
    const int r = hc_pcg(h, o, "lsm_hcond_solve_rhs", f, x, rtol, max_iters, iters, relres);
    if (r != LSM_OK) return r;
    LSM_HIP(h, hipMemcpyAsync(x, o.V.x, (size_t)o.lev[0].nn * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    LSM_HIP(h, hipStreamSynchronize(h->stream));
    return LSM_OK;
}

int lsm_hcond_set_correctors(LsmHcond* s, const double* chi) {
    if (!s) return LSM_ERR_INVALID;
    if (!chi) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_set_correctors: null argument");
    HcondObject& o = *s->o;
    LSM_HIP(s->h, hipMemcpyAsync(o.chi, chi, (size_t)o.N * o.lev[0].nn * sizeof(double), hipMemcpyDefault, s->h->stream));
    LSM_HIP(s->h, hipStreamSynchronize(s->h->stream));
    return LSM_OK;
}

int lsm_hcond_correctors(LsmHcond* s, double* chi_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!chi_out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_correctors: null argument");
    HcondObject& o = *s->o;
    LSM_HIP(s->h, hipMemcpyAsync(chi_out, o.chi, (size_t)o.N * o.lev[0].nn * sizeof(double), hipMemcpyDefault, s->h->stream));
    LSM_HIP(s->h, hipStreamSynchronize(s->h->stream));
    return LSM_OK;
}

int lsm_hcond_energy_cells(LsmHcond* s, int p, int q, double* out) {
    if (!s) return LSM_ERR_INVALID;
    HcondObject& o = *s->o;
    if (!out || p < 0 || q < 0 || p >= o.N || q >= o.N) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_energy_cells: no such pair of unit gradients, or a null array");
    const HcLevel& L = o.lev[0];
    MG_LAUNCH(o.N, hc_energy_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, (const double*)(o.chi + (size_t)p * L.nn),
              (const double*)(o.chi + (size_t)q * L.nn), p, q, out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_hcond_tensor(LsmHcond* s, double* K) {
    if (!s) return LSM_ERR_INVALID;
    if (!K) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_tensor: null argument");
    HcondObject& o = *s->o;
    const HcLevel& L = o.lev[0];
    hipStream_t st = s->h->stream;
    MG_LAUNCH2(o.N, hc_tensor_kernel, 0, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, (const double*)o.chi, (const double*)nullptr, (double*)nullptr, o.tpartial.p,
               &o.st.p->ticket[3], o.sums);
    LSM_HIP(s->h, hipGetLastError());
    LSM_HIP(s->h, hipMemcpyAsync(o.h_sums.p, o.sums, HC_MAXP * sizeof(double), hipMemcpyDeviceToHost, st));
    LSM_HIP(s->h, hipStreamSynchronize(st));
    const int N = o.N;
    for (int q = 0; q < N; ++q)
        for (int p = 0; p <= q; ++p) K[p * N + q] = K[q * N + p] = o.h_sums.p[q * (q + 1) / 2 + p] / (double)L.nn;
    return LSM_OK;
}

int lsm_hcond_corrector(LsmHcond* s, int k, void* u) {
    if (!s) return LSM_ERR_INVALID;
    HcondObject& o = *s->o;
    if (k < 0 || k >= o.N || !u) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_corrector: no such unit gradient, or a null field");
    const HcLevel& L = o.lev[0];
    const long long nnf = (long long)o.G.n[0] * o.G.n[1] * o.G.n[2];
    MG_LAUNCH(o.N, hc_store_kernel, dim3(mg_blocks(nnf)), MG_THREADS, s->h->stream, L, o.G, o.F, (const double*)(o.chi + (size_t)k * L.nn), u);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_hcond_sensitivity(LsmHcond* s, const double* W, void* g_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!W || !g_out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_sensitivity: null argument");
    HcondObject& o = *s->o;
    const int N = o.N;
    for (int p = 0; p < N; ++p)
        for (int q = 0; q < N; ++q)
            if (!std::isfinite(W[p * N + q]) || W[p * N + q] != W[q * N + p]) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_hcond_sensitivity: W must be finite and symmetric");
    const HcLevel& L = o.lev[0];
    hipStream_t st = s->h->stream;
    LSM_HIP(s->h, hipMemcpyAsync(o.W, W, (size_t)N * N * sizeof(double), hipMemcpyHostToDevice, st));
    LSM_HIP(s->h, hipStreamSynchronize(st));      // W is the caller's pageable memory
    MG_LAUNCH2(N, hc_tensor_kernel, 1, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, (const double*)o.chi, (const double*)o.W, o.cell, o.tpartial.p, &o.st.p->ticket[3],
               o.sums);
    const long long nnf = (long long)o.G.n[0] * o.G.n[1] * o.G.n[2];
    MG_LAUNCH(N, hc_sens_gather_kernel, dim3(mg_blocks(nnf)), MG_THREADS, st, L, o.G, o.F, (const double*)o.cell, g_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

void lsm_hcond_destroy(LsmHcond* s) {
    if (!s) return;
    delete s->o;
    delete s;
}
