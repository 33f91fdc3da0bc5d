// lsm_homog.hip — homogenize: the effective elasticity tensor C^H of the periodic material whose cell is the box of ϕ, and its
// sensitivity.  The Q1 operator of lsm_elastic.hip on the torus of the grid's cells (period n − 1 cells: node n − 1 is node 0), the
// M = N(N+1)/2 cell problems A χ^k = f^k solved by mg_pcg.h's conjugate gradients with a wrapping V-cycle, then one pass over the
// cells for the tensor.  DESIGN.md §7.23; include/lsm.h ("homogenize") is the normative text, tests/_homog_ref.py restates it.
// Built with -ffp-contract=off: the cell array, A x, the loads, the cell integrands and the sensitivity round as numpy does.
//
// Storage.  A level has m nodes per axis and as many cells: node I and cell I (the one whose lowest corner is I) share the linear
// index I0 + m0·(I1 + m1·I2).  Solver vectors are fp64, component-major: x[i·nn + id].  The N components of node 0 are pinned to
// zero on every level (fine node 2J = 0 is coarse node 0), which removes the translations; nothing else is fixed.  The correctors
// are kept on the device, M vectors of N·nn doubles; a solve writes them only when all M have converged.
//
// What is mg_pcg.h's: the state, K2, the smoother, the coarsest kernel, the wrapping gather and prolongation (launched through the
// Level), the V-cycle's driver, the iteration loop, the report.  What is this file's own: the wrapping apply (the Level), the load,
// and the cell kernels.
#include <memory>

#include "el_cell.h"
#include "el_k0.h"
#include "mg_pcg.h"

namespace lsm {

static const double HG_OMEGA = 0.6, HG_SAFE = 1.9;      // lsm_elastic.hip's damping rule
enum { HG_BAD_PHI = 0, HG_BAD_E = 1, HG_NSTAT = 4 };
static const int HG_MAXP = 21;      // M(M+1)/2 in 3-D

struct HgVec : MgVec { double* p; };     // the search direction, updated in place
struct HgShape { int n[3]; };            // the handle's dense grid (nodes)
struct HgU { void* p[3]; };

struct HgLevel {
    int n[3];                     // nodes (= cells) of the torus per axis
    int nn;
    double h[3];
    const double* E;              // cell moduli
    const double* D;              // the diagonal, component-major
    const double* K;              // the level's K0, (2^N·N)² row-major
    double om;                    // min(HG_OMEGA, HG_SAFE/λ)

    using Vec = HgVec;
    static constexpr bool wraps = true;
    static constexpr int comps(int N) { return N; }
    __device__ __forceinline__ bool fixed(int id, int) const { return id == 0; }
    __device__ __forceinline__ double omega() const { return om; }
    static void launch_resid(int N, unsigned nb, hipStream_t s, const HgLevel& L, const double* r, const double* x, double* res, const MgState* st);
    static void launch_gather(int N, hipStream_t s, const HgLevel& Lf, const HgLevel& Lc, const int co[3], const double* res, double* rc, const MgState* st);
    static void launch_prolong(int N, hipStream_t s, const HgLevel& Lf, const HgLevel& Lc, const int co[3], const double* xc, double* x, const MgState* st);
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
        const double E = L.E[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
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

// ---- setup of level 0: ϕ checked at every node of the dense grid; the cell moduli from ϕ (el_cell.h: lsm_elastic's array, the same
// bits) or the caller's, checked
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_setup_kernel(HgShape G, MgField F, const void* __restrict__ phi, double level, double e_in, double e_out,
                                                              double hmin, const double* __restrict__ e_given, double* __restrict__ E, unsigned long long* st) {
    unsigned cnt[2] = {0, 0};
    const int nnf = G.n[0] * G.n[1] * G.n[2];
    MG_LOOP(id, nnf) {
        int I[3];
        mg_coords<N>(G.n, id, I);
        if (phi && !mg_finite(ld_val(phi, mg_padded(F, I), F.f32))) ++cnt[HG_BAD_PHI];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && I[d] < G.n[d] - 1;
        if (!corner) continue;
        const int ci = mg_cell_index<N>(G.n, I);
        double ev;
        if (e_given) {
            ev = e_given[ci];
            if (!(ev > 0.0) || !mg_finite(ev)) ++cnt[HG_BAD_E];
        } else {
            ev = el_cell_from_phi<N>(phi, mg_padded(F, I), F.s1, F.s2, F.f32, level, e_in, e_out, hmin);
            if (!(ev > 0.0)) ++cnt[HG_BAD_E];
        }
        E[ci] = ev;
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
__global__ void __launch_bounds__(MG_THREADS) hg_coarsen_kernel(HgLevel Lf, HgLevel Lc, int co0, int co1, int co2, double* __restrict__ Ec) {
    const int co[3] = {co0, co1, co2};
    const int nf[3] = {Lf.n[0] + 1, Lf.n[1] + 1, Lf.n[2] + 1};
    const double scale = mg_coarsen_scale(co0 + co1 + co2);
    MG_LOOP(id, Lc.nn) {
        int J[3];
        mg_coords<N>(Lc.n, id, J);
        Ec[id] = mg_cell_average<N>(Lf.E, nf, J, co, scale);
    }
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
            const double E = L.E[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
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
            const double E = L.E[c[0][m & 1] + c[1][(m >> 1) & 1] + (N > 2 ? c[2][(m >> 2) & 1] : 0)];
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

// ---- PCG
// x₀ = the guess (zero without one) with the pin at zero, p = 0; over the nt unknowns
__global__ void __launch_bounds__(MG_THREADS) hg_start_kernel(int nn, int nt, const double* __restrict__ guess, double* __restrict__ x, double* __restrict__ p) {
    MG_LOOP(t, nt) {
        x[t] = (guess && t % nn != 0) ? guess[t] : 0.0;
        p[t] = 0.0;
    }
}
// r₀ = f − A x₀ away from the pin, 0 there; ‖f_free‖², ‖r₀‖²; jac: z = r/D and ρ = r·z as well
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_init_kernel(HgLevel L, HgVec V, const double* __restrict__ x, const double* __restrict__ f,
                                                             double* __restrict__ rv, double* __restrict__ zv, int jac) {
    double red[4] = {0.0, 0.0, 0.0, 0.0};
    const int nn = L.nn;
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double out[N];
        hg_apply<N>(L, I, [&](int q, int j) { return x[j * nn + q]; }, out);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double ui = x[i * nn + id], fi = f[i * nn + id];
            if (!mg_finite(ui) || !mg_finite(fi)) red[3] += 1.0;
            double r = 0.0, z = 0.0;
            if (id != 0) {
                r = fi - out[i];
                red[0] += fi * fi;
                red[1] += r * r;
                if (jac) {
                    z = r / L.D[i * nn + id];
                    red[2] += r * z;
                }
            }
            rv[i * nn + id] = r;
            if (jac) zv[i * nn + id] = z;
        }
    }
    if (!block_reduce_ordered<4, MG_THREADS>(red, V.partial, &V.st->ticket[0]) || threadIdx.x != 0) return;
    mg_init_tail(*V.st, red, jac);
}
// p = z + β p, in place (both are zero at the pin)
__global__ void __launch_bounds__(MG_THREADS) hg_dir_kernel(int nt, HgVec V) {
    if (V.st->status != MG_RUN) return;
    const double beta = V.st->beta;
    const double* __restrict__ z = V.z;
    double* __restrict__ p = V.p;
    MG_LOOP(k, nt) p[k] = z[k] + beta * p[k];
}
// K1: q = A p, σ = p·q, α = ρ/σ
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_k1_kernel(HgLevel L, const double* __restrict__ p, double* __restrict__ qv, double* partial, MgState* st) {
    if (st->status != MG_RUN) return;
    const int nn = L.nn;
    double red[1] = {0.0};
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double out[N];
        hg_apply<N>(L, I, [&](int q, int j) { return p[j * nn + q]; }, out);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double q = 0.0;
            if (id != 0) {
                q = out[i];
                red[0] += p[i * nn + id] * q;
            }
            qv[i * nn + id] = q;
        }
    }
    if (!block_reduce_ordered<1, MG_THREADS>(red, partial, &st->ticket[1]) || threadIdx.x != 0) return;
    mg_k1_tail(*st, red[0]);
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
        out[id] = L.E[id] * d;
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
        const double E = L.E[id];
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

// s_I = (Σ_C around I of cell[C], ascending, from +0)·2^−N at every node of the handle's grid (node n − 1 is node 0), rounded once
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_sens_gather_kernel(HgLevel L, HgShape G, MgField F, const double* __restrict__ cell, void* __restrict__ g_out) {
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

// χ^k into N fields of the handle, the image nodes n − 1 from node 0, rounded once
template <int N>
__global__ void __launch_bounds__(MG_THREADS) hg_store_kernel(HgLevel L, HgShape G, MgField F, const double* __restrict__ x, HgU U) {
    const int nnf = G.n[0] * G.n[1] * G.n[2];
    MG_LOOP(id, nnf) {
        int I[3], T[3] = {0, 0, 0};
        mg_coords<N>(G.n, id, I);
#pragma unroll
        for (int d = 0; d < N; ++d) T[d] = I[d] == L.n[d] ? 0 : I[d];
        const int tid = T[0] + L.n[0] * (T[1] + (N > 2 ? L.n[1] * T[2] : 0));
        const long long at = mg_padded(F, I);
#pragma unroll
        for (int i = 0; i < N; ++i) st_val(U.p[i], at, F.f32, x[i * L.nn + tid]);
    }
}

// ---- host side
void HgLevel::launch_resid(int N, unsigned nb, hipStream_t s, const HgLevel& L, const double* r, const double* x, double* res, const MgState* st) {
    MG_LAUNCH2(N, mg_resid_kernel, HgLevel, dim3(nb), dim3(MG_THREADS), s, L, r, x, res, st);
}
void HgLevel::launch_gather(int N, hipStream_t s, const HgLevel& Lf, const HgLevel& Lc, const int co[3], const double* res, double* rc, const MgState* st) {
    MG_LAUNCH2(N, mg_wrap_gather_kernel, HgLevel, dim3(mg_blocks(Lc.nn), N), MG_THREADS, s, Lf, Lc, co[0], co[1], co[2], res, rc, st);
}
void HgLevel::launch_prolong(int N, hipStream_t s, const HgLevel& Lf, const HgLevel& Lc, const int co[3], const double* xc, double* x, const MgState* st) {
    MG_LAUNCH2(N, mg_wrap_prolong_kernel, HgLevel, dim3(mg_blocks(Lf.nn), N), MG_THREADS, s, Lf, Lc, co[0], co[1], co[2], xc, x, st);
}

struct HomogObject : MgSolver<HgLevel> {
    std::vector<std::vector<double>> k0;     // the levels' K0 as computed (what the device holds)
    int M = 0;
    HgShape G;                               // the handle's dense grid
    double *chi = nullptr, *chinew = nullptr, *f = nullptr, *cell = nullptr, *chi0 = nullptr, *g = nullptr, *W = nullptr, *sums = nullptr;
    DevBuf<double> tpartial;                 // the tensor kernel's partials: HG_MAXP per workgroup
    PinnedBuf<double> h_sums;
};

// the Voigt pairs in the header's order
static void hg_voigt(int N, int k, int& i, int& j) {
    static const int v2[3][2] = {{0, 0}, {1, 1}, {0, 1}}, v3[6][2] = {{0, 0}, {1, 1}, {2, 2}, {1, 2}, {0, 2}, {0, 1}};
    i = N == 2 ? v2[k][0] : v3[k][0];
    j = N == 2 ? v2[k][1] : v3[k][1];
}

}  // namespace lsm

using namespace lsm;

struct LsmHomog { LsmHandle* h; HomogObject* o; };

static int hg_create(LsmHandle* h, HomogObject& o, const void* phi, double level, double e_in, double e_out, const double* e_cells, double lam, double mu,
                     int64_t stats[4]) {
    const int N = h->grid.ndim;
    o.N = N;
    o.M = N * (N + 1) / 2;
    o.F = MgField{h->lay.stride[1], N > 2 ? h->lay.stride[2] : 0, h->lay.origin, h->dtype == LSM_DTYPE_F32 ? 1 : 0};
    // the hierarchy: axis d coarsens while m_d is even and above 4
    std::vector<HgLevel> lev;
    HgLevel L;
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
    if (nnf >= (1LL << 28)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: the grid is too large (2^28 nodes at most)");
    L.nn = (int)nn;
    lev.push_back(L);
    for (;;) {
        const HgLevel& f = lev.back();
        HgLevel c = f;
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
    const int nl = (int)lev.size(), M = o.M, R = (1 << N) * N;
    const size_t RR = (size_t)R * R, nt = (size_t)N * (size_t)nn;
    // one allocation of doubles: per level K0, cells, D, xa, xb, [rhs]; level 0: x r q p, f, the cell scratch, χ and its staging copy,
    // χ0 and g of every unit strain, W, the tensor's sums
    size_t nd = 0;
    for (int l = 0; l < nl; ++l) nd += RR + (size_t)lev[l].nn + (size_t)N * (size_t)lev[l].nn * (size_t)(3 + (l ? 1 : 4));
    nd += nt + (size_t)nn + 2 * (size_t)M * nt + 2 * (size_t)M * R + (size_t)M * M + HG_MAXP;
    LSM_HIP(h, o.buf.alloc(nd * sizeof(double)));
    LSM_HIP(h, o.tpartial.alloc((size_t)HG_MAXP * MG_MAXB * sizeof(double)));
    LSM_HIP(h, o.h_sums.alloc(HG_MAXP * sizeof(double)));
    hipStream_t s = h->stream;
    const int ra = mg_alloc_scalars(h, o, HG_NSTAT, s);
    if (ra != LSM_OK) return ra;
    double* b = o.buf;
    std::vector<double*> ecell(nl), dg(nl), kd(nl);
    o.rhs.assign(nl, nullptr); o.xa.assign(nl, nullptr); o.xb.assign(nl, nullptr);
    o.k0.resize(nl);
    for (int l = 0; l < nl; ++l) {
        const size_t m = (size_t)N * (size_t)lev[l].nn;
        kd[l] = b; b += RR;
        ecell[l] = b; b += lev[l].nn;
        dg[l] = b; b += m;
        o.xa[l] = b; b += m;
        o.xb[l] = b; b += m;
        if (l) { o.rhs[l] = b; b += m; }
        else {
            o.V.x = b; b += m; o.V.r = b; b += m; o.V.q = b; b += m; o.V.p = b; b += m;
        }
        lev[l].E = ecell[l]; lev[l].D = dg[l]; lev[l].K = kd[l];
        es_k0(N, lev[l].h, lam, mu, o.k0[l]);
        lev[l].om = std::min(HG_OMEGA, HG_SAFE / es_symbol_lambda(N, o.k0[l]));
        LSM_HIP(h, hipMemcpyAsync(kd[l], o.k0[l].data(), RR * sizeof(double), hipMemcpyHostToDevice, s));
    }
    o.f = b; b += nt;
    o.cell = b; b += nn;
    o.chi = b; b += (size_t)M * nt;
    o.chinew = b; b += (size_t)M * nt;
    o.chi0 = b; b += (size_t)M * R;
    o.g = b; b += (size_t)M * R;
    o.W = b; b += (size_t)M * M;
    o.sums = b; b += HG_MAXP;
    LSM_HIP(h, hipMemsetAsync(o.chi, 0, (size_t)M * nt * sizeof(double), s));
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
    MG_LAUNCH(N, hg_setup_kernel, dim3(mg_blocks(nnf)), MG_THREADS, s, o.G, o.F, e_cells ? (const void*)nullptr : phi, level, e_in, e_out, hmin, e_cells, ecell[0],
              o.cnt.p);
    LSM_HIP(h, hipGetLastError());
    unsigned long long c[HG_NSTAT] = {};
    LSM_HIP(h, hipMemcpyAsync(c, o.cnt.p, sizeof(c), hipMemcpyDeviceToHost, s));
    LSM_HIP(h, hipStreamSynchronize(s));      // c0 and g are read by now
    const int reason = c[HG_BAD_PHI] ? 1 : c[HG_BAD_E] ? 2 : 0;
    if (reason) {
        if (stats) { stats[0] = -reason; stats[1] = (int64_t)(reason == 1 ? c[HG_BAD_PHI] : c[HG_BAD_E]); stats[2] = stats[3] = 0; }
        return lsm_fail(h, LSM_ERR_INVALID, reason == 1 ? "lsm_homog_create: phi must be finite" : "lsm_homog_create: the cell moduli must be finite and positive");
    }
    for (int l = 1; l < nl; ++l)
        MG_LAUNCH(N, hg_coarsen_kernel, dim3(mg_blocks(lev[l].nn)), MG_THREADS, s, lev[l - 1], lev[l], o.co[l - 1][0], o.co[l - 1][1], o.co[l - 1][2], ecell[l]);
    for (int l = 0; l < nl; ++l) MG_LAUNCH(N, hg_diag_kernel, dim3(mg_blocks(lev[l].nn)), MG_THREADS, s, lev[l], dg[l]);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(s));
    o.lev = lev;
    o.nfixed = N;
    o.nfree = (long long)nt - N;
    o.V.z = o.precond == LSM_PRECOND_JACOBI ? o.xa[0] : o.xb[0];
    if (stats) { stats[0] = nl; stats[1] = o.nfree; stats[2] = nn; stats[3] = 0; }
    return LSM_OK;
}

int lsm_homog_create(LsmHandle* h, const void* phi, double level, double e_in, double e_out, const double* e_cells, double nu, int plane, int precond,
                     LsmHomog** out, int64_t stats[4]) {
    if (!h || !out) return h ? lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: null argument") : LSM_ERR_INVALID;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (!phi && !e_cells) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: give phi or the cell moduli");
    const int N = h->grid.ndim;
    if (N == 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: a 1-dimensional grid is not supported (2-D and 3-D only)");
    if (h->comm) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: the handle has a communicator attached (single device only)");
    if (h->bc[N - 1][0].kind == LSM_BC_NONE || h->bc[N - 1][1].kind == LSM_BC_NONE)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: the handle is a slab of a multi-GPU grid (whole grids only)");
    for (int d = 0; d < N; ++d)
        if (h->nloc[d] < 3) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: at least 3 nodes (2 cells) per dimension");
    if (!e_cells && (!(e_in > 0) || !std::isfinite(e_in) || !(e_out > 0) || !std::isfinite(e_out)))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: e_in and e_out must be finite and positive");
    if (!e_cells && !std::isfinite(level)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: level must be finite");
    if (!std::isfinite(nu) || !(nu > -1.0) || !(nu < 0.5)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: nu must be finite with -1 < nu < 0.5");
    if (plane != LSM_PLANE_STRESS && plane != LSM_PLANE_STRAIN) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: unknown plane (LSM_PLANE_STRESS or LSM_PLANE_STRAIN)");
    if (precond != LSM_PRECOND_MG && precond != LSM_PRECOND_JACOBI) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_create: unknown preconditioner");
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

int lsm_homog_cells(LsmHomog* s, double* e_out_cells) {
    if (!s) return LSM_ERR_INVALID;
    if (!e_out_cells) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_cells: null argument");
    const HgLevel& L = s->o->lev[0];
    LSM_HIP(s->h, hipMemcpyAsync(e_out_cells, L.E, (size_t)L.nn * sizeof(double), hipMemcpyDeviceToDevice, s->h->stream));
    return LSM_OK;
}

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
    HomogObject& o = *s->o;
    if (!f_out || k < 0 || k >= o.M) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_load: no such unit strain, or a null array");
    const HgLevel& L = o.lev[0];
    MG_LAUNCH(o.N, hg_load_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, (const double*)(o.g + (size_t)k * (1 << o.N) * o.N), f_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

// A x = f away from the pin by PCG from `guess` (device, N·nn; NULL: zero); the solution is left in o.V.x
static int hg_pcg(LsmHandle* h, HomogObject& o, const char* fn, const double* f, const double* guess, double rtol, int max_iters, int* iters, double* relres) {
    const int N = o.N;
    const HgLevel& L = o.lev[0];
    const int jac = o.precond == LSM_PRECOND_JACOBI;
    hipStream_t st = h->stream;
    const unsigned nb = mg_blocks(L.nn), nbt = mg_blocks((long long)N * L.nn);
    const int nt = N * L.nn;
    const int r0 = mg_reset(h, o, rtol, max_iters, st);
    if (r0 != LSM_OK) return r0;
    hipLaunchKernelGGL(hg_start_kernel, dim3(nbt), dim3(MG_THREADS), 0, st, L.nn, nt, guess, o.V.x, o.V.p);
    MG_LAUNCH(N, hg_init_kernel, dim3(nb), MG_THREADS, st, L, o.V, (const double*)o.V.x, f, o.V.r, o.V.z, jac);
    LSM_HIP(h, hipGetLastError());
    const int r1 = mg_iterate(h, o, max_iters, st, [&](int) {
        if (!jac) mg_vcycle(o, o.V.r, st);
        hipLaunchKernelGGL(hg_dir_kernel, dim3(nbt), dim3(MG_THREADS), 0, st, nt, o.V);
        MG_LAUNCH(N, hg_k1_kernel, dim3(nb), MG_THREADS, st, L, (const double*)o.V.p, o.V.q, o.partial.p, o.st.p);
        if (jac) hipLaunchKernelGGL(mg_k2_kernel<1>, dim3(nbt), dim3(MG_THREADS), 0, st, L.D, nt, (MgVec)o.V, (const double*)o.V.p);
        else hipLaunchKernelGGL(mg_k2_kernel<0>, dim3(nbt), dim3(MG_THREADS), 0, st, L.D, nt, (MgVec)o.V, (const double*)o.V.p);
    });
    if (r1 != LSM_OK) return r1;
    return mg_report(h, o, fn, rtol, iters, relres);
}

int lsm_homog_solve(LsmHomog* s, const double* chi_guess, double rtol, int max_iters, int* iters, double* relres) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    HomogObject& o = *s->o;
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_solve: rtol must be positive and max_iters at least 1");
    const int N = o.N, M = o.M;
    const HgLevel& L = o.lev[0];
    (void)hipSetDevice(h->device);
    hipStream_t st = h->stream;
    const size_t nt = (size_t)N * L.nn;
    for (int k = 0; k < M; ++k) {
        if (iters) iters[k] = 0;
        if (relres) relres[k] = 0.0;
    }
    const double* guess = nullptr;
    if (chi_guess) {      // the caller's memory, host or device: staged where the new correctors will land
        LSM_HIP(h, hipMemcpyAsync(o.chinew, chi_guess, (size_t)M * nt * sizeof(double), hipMemcpyDefault, st));
        LSM_HIP(h, hipStreamSynchronize(st));
        guess = o.chinew;
    }
    for (int k = 0; k < M; ++k) {
        MG_LAUNCH(N, hg_load_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, (const double*)(o.g + (size_t)k * (1 << N) * N), o.f);
        const int r = hg_pcg(h, o, "lsm_homog_solve", o.f, guess ? guess + k * nt : nullptr, rtol, max_iters, iters ? iters + k : nullptr, relres ? relres + k : nullptr);
        if (r != LSM_OK) return r;      // the stored correctors are untouched
        LSM_HIP(h, hipMemcpyAsync(o.chinew + k * nt, o.V.x, nt * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    LSM_HIP(h, hipMemcpyAsync(o.chi, o.chinew, (size_t)M * nt * sizeof(double), hipMemcpyDeviceToDevice, st));
    LSM_HIP(h, hipStreamSynchronize(st));
    return LSM_OK;
}

int lsm_homog_solve_rhs(LsmHomog* s, const double* f, double* x, double rtol, int max_iters, int* iters, double* relres) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    HomogObject& o = *s->o;
    if (!f || !x || f == x) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_solve_rhs: f and x must be two arrays");
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_homog_solve_rhs: rtol must be positive and max_iters at least 1");
    (void)hipSetDevice(h->device);
    const int r = hg_pcg(h, o, "lsm_homog_solve_rhs", f, x, rtol, max_iters, iters, relres);
    if (r != LSM_OK) return r;
    LSM_HIP(h, hipMemcpyAsync(x, o.V.x, (size_t)o.N * o.lev[0].nn * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    LSM_HIP(h, hipStreamSynchronize(h->stream));
    return LSM_OK;
}

int lsm_homog_set_correctors(LsmHomog* s, const double* chi) {
    if (!s) return LSM_ERR_INVALID;
    if (!chi) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_set_correctors: null argument");
    HomogObject& o = *s->o;
    const size_t nt = (size_t)o.N * o.lev[0].nn;
    LSM_HIP(s->h, hipMemcpyAsync(o.chi, chi, (size_t)o.M * nt * sizeof(double), hipMemcpyDefault, s->h->stream));
    LSM_HIP(s->h, hipStreamSynchronize(s->h->stream));
    return LSM_OK;
}

int lsm_homog_correctors(LsmHomog* s, double* chi_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!chi_out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_correctors: null argument");
    HomogObject& o = *s->o;
    const size_t nt = (size_t)o.N * o.lev[0].nn;
    LSM_HIP(s->h, hipMemcpyAsync(chi_out, o.chi, (size_t)o.M * nt * sizeof(double), hipMemcpyDefault, s->h->stream));
    LSM_HIP(s->h, hipStreamSynchronize(s->h->stream));
    return LSM_OK;
}

int lsm_homog_energy_cells(LsmHomog* s, int p, int q, double* out) {
    if (!s) return LSM_ERR_INVALID;
    HomogObject& o = *s->o;
    if (!out || p < 0 || q < 0 || p >= o.M || q >= o.M) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_energy_cells: no such pair of unit strains, or a null array");
    const HgLevel& L = o.lev[0];
    const size_t nt = (size_t)o.N * L.nn, R = (size_t)(1 << o.N) * o.N;
    MG_LAUNCH(o.N, hg_energy_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, (const double*)(o.chi + p * nt), (const double*)(o.chi + q * nt),
              (const double*)(o.chi0 + p * R), (const double*)(o.chi0 + q * R), out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_homog_tensor(LsmHomog* s, double* C) {
    if (!s) return LSM_ERR_INVALID;
    if (!C) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_tensor: null argument");
    HomogObject& o = *s->o;
    const HgLevel& L = o.lev[0];
    hipStream_t st = s->h->stream;
    MG_LAUNCH2(o.N, hg_tensor_kernel, 0, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, (const double*)o.chi, (const double*)o.chi0, (const double*)nullptr, (double*)nullptr,
               o.tpartial.p, &o.st.p->ticket[3], o.sums);
    LSM_HIP(s->h, hipGetLastError());
    LSM_HIP(s->h, hipMemcpyAsync(o.h_sums.p, o.sums, HG_MAXP * sizeof(double), hipMemcpyDeviceToHost, st));
    LSM_HIP(s->h, hipStreamSynchronize(st));
    const int M = o.M;
    for (int q = 0; q < M; ++q)
        for (int p = 0; p <= q; ++p) C[p * M + q] = C[q * M + p] = o.h_sums.p[q * (q + 1) / 2 + p] / (double)L.nn;
    return LSM_OK;
}

int lsm_homog_corrector(LsmHomog* s, int k, void* u0, void* u1, void* u2) {
    if (!s) return LSM_ERR_INVALID;
    HomogObject& o = *s->o;
    HgU U;
    U.p[0] = u0; U.p[1] = u1; U.p[2] = o.N > 2 ? u2 : nullptr;
    if (k < 0 || k >= o.M || !u0 || !u1 || u0 == u1 || (o.N > 2 && (!u2 || u2 == u0 || u2 == u1)))
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_corrector: no such unit strain, or the N fields are not distinct");
    const HgLevel& L = o.lev[0];
    const long long nnf = (long long)o.G.n[0] * o.G.n[1] * o.G.n[2];
    MG_LAUNCH(o.N, hg_store_kernel, dim3(mg_blocks(nnf)), MG_THREADS, s->h->stream, L, o.G, o.F, (const double*)(o.chi + (size_t)k * o.N * L.nn), U);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_homog_sensitivity(LsmHomog* s, const double* W, void* g_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!W || !g_out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_sensitivity: null argument");
    HomogObject& o = *s->o;
    const int M = o.M;
    for (int p = 0; p < M; ++p)
        for (int q = 0; q < M; ++q)
            if (!std::isfinite(W[p * M + q]) || W[p * M + q] != W[q * M + p]) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_homog_sensitivity: W must be finite and symmetric");
    const HgLevel& L = o.lev[0];
    hipStream_t st = s->h->stream;
    LSM_HIP(s->h, hipMemcpyAsync(o.W, W, (size_t)M * M * sizeof(double), hipMemcpyHostToDevice, st));
    LSM_HIP(s->h, hipStreamSynchronize(st));      // W is the caller's pageable memory
    MG_LAUNCH2(o.N, hg_tensor_kernel, 1, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, (const double*)o.chi, (const double*)o.chi0, (const double*)o.W, o.cell, o.tpartial.p,
               &o.st.p->ticket[3], o.sums);
    const long long nnf = (long long)o.G.n[0] * o.G.n[1] * o.G.n[2];
    MG_LAUNCH(o.N, hg_sens_gather_kernel, dim3(mg_blocks(nnf)), MG_THREADS, st, L, o.G, o.F, (const double*)o.cell, g_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

void lsm_homog_destroy(LsmHomog* s) {
    if (!s) return;
    delete s->o;
    delete s;
}
