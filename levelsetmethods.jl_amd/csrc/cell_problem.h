// cell_problem.h — the periodic cell problems that lsm_homog.hip (homogenize) and lsm_hcond.hip (homogenize_conductivity) share: an
// operator on the torus of the grid's cells (period n − 1 cells: node n − 1 is node 0), K cell problems A χ^k = f^k solved one after
// the other by mg_pcg.h's conjugate gradients with a wrapping V-cycle, the new correctors staged and committed only when all K have
// converged, then one pass over the cells for the tensor, the same pass without the reduction for the sensitivity, and the gather of
// the cell values to the handle's nodes.  An operator's file brings its Level (a CpLevel with comps, omega and apply), its diagonal,
// load, energy and tensor kernels; everything here is written once over the Level.  Both files are built with -ffp-contract=off
// and this header inherits that.  DESIGN.md §7.23 (elasticity), §7.24 (conductivity).
//
// Storage.  A level has m nodes per axis and as many cells: node I and cell I (the one whose lowest corner is I) share the linear
// index I0 + m0·(I1 + m1·I2).  Solver vectors are fp64, component-major: x[i·nn + id], comps(N) components.  The components of
// node 0 are pinned to zero on every level (fine node 2J = 0 is coarse node 0), which removes the null space; nothing else is
// fixed.  The correctors are kept on the device, K vectors of comps·nn doubles.
//
// Messages carry the C entry point's name in front (fn), so each file's refusals read as they always did.
#pragma once

#include "el_cell.h"
#include "mg_pcg.h"

namespace lsm {

enum { CP_BAD_PHI = 0, CP_BAD_CELL = 1, CP_NSTAT = 4 };

struct CpVec : MgVec { double* p; };     // the search direction, updated in place
struct CpShape { int n[3]; };            // the handle's dense grid (nodes)
struct CpFields { void* p[3]; };         // the comps(N) fields of the handle that take a corrector

// ---- the index arithmetic of a grid that wraps: n nodes (= cells) per axis, node n is node 0
// c[d][o + 1] = ((I_d + o) mod n_d)·(the axis' stride), o ∈ {−1, 0, 1}: nodes and cells share it
template <int N>
__device__ __forceinline__ void mg_wrapped(const int n[3], const int I[3], int c[3][3]) {
    const int st[3] = {1, n[0], n[0] * n[1]};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (d < N) {
            c[d][0] = (I[d] == 0 ? n[d] - 1 : I[d] - 1) * st[d];
            c[d][1] = I[d] * st[d];
            c[d][2] = (I[d] == n[d] - 1 ? 0 : I[d] + 1) * st[d];
        } else c[d][0] = c[d][1] = c[d][2] = 0;
    }
}
// the 2^N corner nodes of cell C, wrapped
template <int N>
__device__ __forceinline__ void mg_wrapped_corners(const int n[3], const int C[3], int node[1 << N]) {
    int up[3] = {0, 0, 0};
#pragma unroll
    for (int d = 0; d < N; ++d) up[d] = C[d] == n[d] - 1 ? 0 : C[d] + 1;
#pragma unroll
    for (int b = 0; b < (1 << N); ++b)
        node[b] = ((b & 1) ? up[0] : C[0]) + n[0] * (((b >> 1) & 1 ? up[1] : C[1]) + (N > 2 ? n[1] * ((b >> 2) & 1 ? up[2] : C[2]) : 0));
}

// ---- the transfers of a grid that wraps (m nodes per axis, node m is node 0, m even on a coarsened axis), per component
// (blockIdx.y).  r_c[J] = 2^−k·Σ_o w_o·res[(2J + o) mod m], w = 1 at o = 0 and ½ at o = ±1 per coarsened axis (o0 fastest, from +0);
// zero on the fixed components (the pin)
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) mg_wrap_gather_kernel(Level Lf, Level Lc, int co0, int co1, int co2, const double* __restrict__ res,
                                                                    double* __restrict__ rc, const MgState* st) {
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
                    if (I[d] < 0) I[d] += Lf.n[d];
                    if (I[d] >= Lf.n[d]) I[d] -= Lf.n[d];
                    if (o[d] != 0) w = w * 0.5;
                }
                if (use) acc += w * res[I[0] + Lf.n[0] * (I[1] + (N > 2 ? Lf.n[1] * I[2] : 0))];     // zero on fixed fine components
            }
        }
        rc[id] = acc * scale;
    }
}
// x += P x_c on the free fine components: the transpose of the wrapping gather without its 2^−k
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) mg_wrap_prolong_kernel(Level Lf, Level Lc, int co0, int co1, int co2, const double* __restrict__ xc,
                                                                     double* __restrict__ x, const MgState* st) {
    if (st->status != MG_RUN) return;
    const int co[3] = {co0, co1, co2};
    const int comp = blockIdx.y;
    xc += (size_t)comp * Lc.nn;
    x += (size_t)comp * Lf.nn;
    MG_LOOP(id, Lf.nn) {
        if (Lf.fixed(id, comp)) continue;
        int I[3];
        mg_coords<N>(Lf.n, id, I);
        int J0[3] = {0, 0, 0}, J1[3] = {0, 0, 0}, two[3] = {0, 0, 0};
#pragma unroll
        for (int d = 0; d < N; ++d) {
            J0[d] = co[d] ? I[d] >> 1 : I[d];
            two[d] = co[d] && (I[d] & 1);
            J1[d] = J0[d] + 1 == Lc.n[d] ? 0 : J0[d] + 1;
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
                J[d] = b ? J1[d] : J0[d];
            }
            if (use) acc += w * xc[J[0] + Lc.n[0] * (J[1] + (N > 2 ? Lc.n[1] * J[2] : 0))];
        }
        x[id] = x[id] + acc;
    }
}

// ---- what the two Levels have in common, without data (the fields stay the Level's own, so its kernels compile as they did).
// Level, the derived struct, has
//   int n[3], nn; double h[3]          nodes (= cells) of the torus per axis, their count, the spacings
//   const double *cell, *D             the cells' coefficient (moduli, conductivities); the diagonal, component-major
//   static constexpr int comps(int N),  double omega(),  apply<N, MASK>(id, I, x, stride, out)
//   bool fixed(id, comp)               id == 0: the pin.  x holds zero there, so apply has nothing to mask
template <class Level>
struct CpLevel {
    using Vec = CpVec;
    static constexpr bool wraps = true;
    static void launch_resid(int N, unsigned nb, hipStream_t s, const Level& L, const double* r, const double* x, double* res, const MgState* st) {
        MG_LAUNCH2(N, mg_resid_kernel, Level, dim3(nb), dim3(MG_THREADS), s, L, r, x, res, st);
    }
    static void launch_gather(int N, hipStream_t s, const Level& Lf, const Level& Lc, const int co[3], const double* res, double* rc, const MgState* st) {
        MG_LAUNCH2(N, mg_wrap_gather_kernel, Level, dim3(mg_blocks(Lc.nn), Level::comps(N)), MG_THREADS, s, Lf, Lc, co[0], co[1], co[2], res, rc, st);
    }
    static void launch_prolong(int N, hipStream_t s, const Level& Lf, const Level& Lc, const int co[3], const double* xc, double* x, const MgState* st) {
        MG_LAUNCH2(N, mg_wrap_prolong_kernel, Level, dim3(mg_blocks(Lf.nn), Level::comps(N)), MG_THREADS, s, Lf, Lc, co[0], co[1], co[2], xc, x, st);
    }
};

// ---- setup of level 0: ϕ checked at every node of the dense grid; the cells from ϕ (el_cell.h: the array of lsm_elastic and
// lsm_elliptic, the same bits) or the caller's, checked
template <int N>
__global__ void __launch_bounds__(MG_THREADS) cp_setup_kernel(CpShape G, MgField F, const void* __restrict__ phi, double level, double v_in, double v_out,
                                                              double hmin, const double* __restrict__ given, double* __restrict__ cell, unsigned long long* st) {
    unsigned cnt[2] = {0, 0};
    const int nnf = G.n[0] * G.n[1] * G.n[2];
    MG_LOOP(id, nnf) {
        int I[3];
        mg_coords<N>(G.n, id, I);
        if (phi && !mg_finite(ld_val(phi, mg_padded(F, I), F.f32))) ++cnt[CP_BAD_PHI];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && I[d] < G.n[d] - 1;
        if (!corner) continue;
        const int ci = mg_cell_index<N>(G.n, I);
        double v;
        if (given) {
            v = given[ci];
            if (!(v > 0.0) || !mg_finite(v)) ++cnt[CP_BAD_CELL];
        } else {
            v = el_cell_from_phi<N>(phi, mg_padded(F, I), F.s1, F.s2, F.f32, level, v_in, v_out, hmin);
            if (!(v > 0.0)) ++cnt[CP_BAD_CELL];
        }
        cell[ci] = v;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned v = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&st[k], (unsigned long long)v);
    }
}

// ---- a coarse level's cells: mg_cell_average of the cells {2J, 2J+1} per coarsened axis (a level with m cells per axis is
// mg_cell_index's grid of m + 1 nodes)
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) cp_coarsen_kernel(Level Lf, Level Lc, int co0, int co1, int co2, double* __restrict__ cc) {
    const int co[3] = {co0, co1, co2};
    const int nf[3] = {Lf.n[0] + 1, Lf.n[1] + 1, Lf.n[2] + 1};
    const double scale = mg_coarsen_scale(co0 + co1 + co2);
    MG_LOOP(id, Lc.nn) {
        int J[3];
        mg_coords<N>(Lc.n, id, J);
        cc[id] = mg_cell_average<N>(Lf.cell, nf, J, co, scale);
    }
}

// ---- PCG
// x₀ = the guess (zero without one) with the pin at zero, p = 0; over the nt unknowns.  (static: no template, and two files include this)
static __global__ void __launch_bounds__(MG_THREADS) cp_start_kernel(int nn, int nt, const double* __restrict__ guess, double* __restrict__ x, double* __restrict__ p) {
    MG_LOOP(t, nt) {
        x[t] = (guess && t % nn != 0) ? guess[t] : 0.0;
        p[t] = 0.0;
    }
}
// r₀ = f − A x₀ away from the pin, 0 there; ‖f_free‖², ‖r₀‖²; jac: z = r/D and ρ = r·z as well.  Components ascending within a node
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) cp_init_kernel(Level L, CpVec V, const double* __restrict__ x, const double* __restrict__ f,
                                                             double* __restrict__ rv, double* __restrict__ zv, int jac) {
    constexpr int NC = Level::comps(N);
    double red[4] = {0.0, 0.0, 0.0, 0.0};
    const int nn = L.nn;
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double out[NC];
        L.template apply<N, false>(id, I, x, nn, out);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
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
static __global__ void __launch_bounds__(MG_THREADS) cp_dir_kernel(int nt, CpVec V) {
    if (V.st->status != MG_RUN) return;
    const double beta = V.st->beta;
    const double* __restrict__ z = V.z;
    double* __restrict__ p = V.p;
    MG_LOOP(k, nt) p[k] = z[k] + beta * p[k];
}
// K1: q = A p, σ = p·q, α = ρ/σ
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) cp_k1_kernel(Level L, const double* __restrict__ p, double* __restrict__ qv, double* partial, MgState* st) {
    if (st->status != MG_RUN) return;
    constexpr int NC = Level::comps(N);
    const int nn = L.nn;
    double red[1] = {0.0};
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double out[NC];
        L.template apply<N, false>(id, I, p, nn, out);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
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

// s_I = (Σ_C around I of cell[C], ascending, from +0)·2^−N at every node of the handle's grid (node n − 1 is node 0), rounded once
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) cp_sens_gather_kernel(Level L, CpShape G, MgField F, const double* __restrict__ cell, void* __restrict__ g_out) {
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

// a corrector into comps(N) fields of the handle, the image nodes n − 1 from node 0, rounded once
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) cp_store_kernel(Level L, CpShape G, MgField F, const double* __restrict__ x, CpFields U) {
    const int nnf = G.n[0] * G.n[1] * G.n[2];
    MG_LOOP(id, nnf) {
        int I[3], T[3] = {0, 0, 0};
        mg_coords<N>(G.n, id, I);
#pragma unroll
        for (int d = 0; d < N; ++d) T[d] = I[d] == L.n[d] ? 0 : I[d];
        const int tid = T[0] + L.n[0] * (T[1] + (N > 2 ? L.n[1] * T[2] : 0));
        const long long at = mg_padded(F, I);
#pragma unroll
        for (int i = 0; i < Level::comps(N); ++i) st_val(U.p[i], at, F.f32, x[i * L.nn + tid]);
    }
}

// ---- host side
template <class Level>
struct CellProblem : MgSolver<Level> {
    int K = 0, NP = 0;                       // the cell problems; the pairs p ≤ q that the tensor kernel reduces, K(K+1)/2
    CpShape G;                               // the handle's dense grid
    double *chi = nullptr, *chinew = nullptr, *f = nullptr, *cell = nullptr, *W = nullptr, *sums = nullptr;
    DevBuf<double> tpartial;                 // the tensor kernel's partials: NP per workgroup
    PinnedBuf<double> h_sums;
    size_t nt() const { return (size_t)Level::comps(this->N) * this->lev[0].nn; }      // the unknowns of one cell problem
    long long nnf() const { return (long long)G.n[0] * G.n[1] * G.n[2]; }
};

// where cp_alloc put what the setup writes: per level the cells, the diagonal and the operator's own doubles; own[nl]: its tail
struct CpCarve { std::vector<double*> cells, diag, own; };

// the torus hierarchy from the handle's grid: o.N, o.F, o.G, o.co and n, h, nn of every level (the operator's own fields zero).
// Axis d coarsens while m_d is even and above 4, to m_d/2 with 2h; it ends when no axis coarsens (31 levels at most).  Leaves lev
// empty when the dense grid has max_nodes or more; hmin: the smallest spacing of level 0
template <class Level>
static void cp_shapes(const LsmHandle* h, CellProblem<Level>& o, long long max_nodes, std::vector<Level>& lev, double& hmin) {
    const int N = o.N = h->grid.ndim;
    o.F = MgField{h->lay.stride[1], N > 2 ? h->lay.stride[2] : 0, h->lay.origin, h->dtype == LSM_DTYPE_F32 ? 1 : 0};
    Level L;
    memset(&L, 0, sizeof(L));
    long long nn = 1;
    hmin = INFINITY;
    for (int d = 0; d < 3; ++d) {
        o.G.n[d] = d < N ? h->nloc[d] : 1;
        L.n[d] = d < N ? h->nloc[d] - 1 : 1;
        L.h[d] = d < N ? h->h[d] : 1.0;
        nn *= L.n[d];
        if (d < N) hmin = std::min(hmin, L.h[d]);
    }
    lev.clear();
    if (o.nnf() >= max_nodes) return;
    L.nn = (int)nn;
    lev.push_back(L);
    for (;;) {
        const Level& f = lev.back();
        Level c = f;
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
}

// one allocation of doubles, carved: per level [own_level of the operator's], cells, D, xa, xb, [rhs]; level 0: x r q p; then f, the
// cell scratch, χ (zero) and its staging copy, W, the tensor's sums, [own_tail of the operator's].  o.K is set by now
template <class Level>
static int cp_alloc(LsmHandle* h, CellProblem<Level>& o, std::vector<Level>& lev, size_t own_level, size_t own_tail, CpCarve& c) {
    const int N = o.N, nl = (int)lev.size(), K = o.K, nc = Level::comps(N);
    const size_t nn = (size_t)lev[0].nn, nt = (size_t)nc * nn;
    o.NP = K * (K + 1) / 2;
    size_t nd = 0;
    for (int l = 0; l < nl; ++l) nd += own_level + (size_t)lev[l].nn + (size_t)nc * (size_t)lev[l].nn * (size_t)(3 + (l ? 1 : 4));
    nd += nt + nn + 2 * (size_t)K * nt + (size_t)K * K + o.NP + own_tail;
    LSM_HIP(h, o.buf.alloc(nd * sizeof(double)));
    LSM_HIP(h, o.tpartial.alloc((size_t)o.NP * MG_MAXB * sizeof(double)));
    LSM_HIP(h, o.h_sums.alloc(o.NP * sizeof(double)));
    const int ra = mg_alloc_scalars(h, o, CP_NSTAT, h->stream);
    if (ra != LSM_OK) return ra;
    double* b = o.buf;
    c.cells.assign(nl, nullptr); c.diag.assign(nl, nullptr); c.own.assign(nl + 1, nullptr);
    o.rhs.assign(nl, nullptr); o.xa.assign(nl, nullptr); o.xb.assign(nl, nullptr);
    for (int l = 0; l < nl; ++l) {
        const size_t m = (size_t)nc * (size_t)lev[l].nn;
        c.own[l] = b; b += own_level;
        c.cells[l] = b; b += lev[l].nn;
        c.diag[l] = b; b += m;
        o.xa[l] = b; b += m;
        o.xb[l] = b; b += m;
        if (l) { o.rhs[l] = b; b += m; }
        else {
            o.V.x = b; b += m; o.V.r = b; b += m; o.V.q = b; b += m; o.V.p = b; b += m;
        }
        lev[l].cell = c.cells[l]; lev[l].D = c.diag[l];
    }
    o.f = b; b += nt;
    o.cell = b; b += nn;
    o.chi = b; b += (size_t)K * nt;
    o.chinew = b; b += (size_t)K * nt;
    o.W = b; b += (size_t)K * K;
    o.sums = b; b += o.NP;
    c.own[nl] = b;
    LSM_HIP(h, hipMemsetAsync(o.chi, 0, (size_t)K * nt * sizeof(double), h->stream));
    return LSM_OK;
}

// the cells of level 0 from ϕ or from `given`, refused when ϕ is not finite or a cell is not finite and positive (`cells`: what the
// message calls them); then the coarse levels' cells and every level's diagonal by diag(level, D); the solver's counts; the stats
template <class Level, class Diag>
static int cp_setup(LsmHandle* h, CellProblem<Level>& o, std::vector<Level>& lev, const CpCarve& c, const char* fn, const char* cells, const void* phi, double level,
                    double v_in, double v_out, const double* given, double hmin, int64_t stats[4], Diag diag) {
    const int N = o.N, nl = (int)lev.size();
    hipStream_t s = h->stream;
    MG_LAUNCH(N, cp_setup_kernel, dim3(mg_blocks(o.nnf())), MG_THREADS, s, o.G, o.F, given ? (const void*)nullptr : phi, level, v_in, v_out, hmin, given, c.cells[0],
              o.cnt.p);
    LSM_HIP(h, hipGetLastError());
    unsigned long long cnt[CP_NSTAT] = {};
    LSM_HIP(h, hipMemcpyAsync(cnt, o.cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, s));
    LSM_HIP(h, hipStreamSynchronize(s));      // what the caller uploaded from its own vectors is read by now
    const int reason = cnt[CP_BAD_PHI] ? 1 : cnt[CP_BAD_CELL] ? 2 : 0;
    if (reason) {
        if (stats) { stats[0] = -reason; stats[1] = (int64_t)(reason == 1 ? cnt[CP_BAD_PHI] : cnt[CP_BAD_CELL]); stats[2] = stats[3] = 0; }
        return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + (reason == 1 ? ": phi must be finite" : std::string(": the cell ") + cells + " must be finite and positive"));
    }
    for (int l = 1; l < nl; ++l)
        MG_LAUNCH2(N, cp_coarsen_kernel, Level, dim3(mg_blocks(lev[l].nn)), MG_THREADS, s, lev[l - 1], lev[l], o.co[l - 1][0], o.co[l - 1][1], o.co[l - 1][2], c.cells[l]);
    for (int l = 0; l < nl; ++l) diag(lev[l], c.diag[l]);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(s));
    o.lev = lev;
    o.nfixed = Level::comps(N);
    o.nfree = (long long)o.nt() - o.nfixed;
    o.V.z = o.precond == LSM_PRECOND_JACOBI ? o.xa[0] : o.xb[0];
    if (stats) { stats[0] = nl; stats[1] = o.nfree; stats[2] = lev[0].nn; stats[3] = 0; }
    return LSM_OK;
}

// the refusals of create that the two share, in their order; in, out: the names of the two values (e_in, e_out)
static int cp_create_check(LsmHandle* h, const void* out, int64_t stats[4], const char* fn, const char* cells, const char* in, const char* outn, const void* phi,
                           const double* given, double level, double v_in, double v_out) {
    const std::string f = std::string(fn) + ": ";
    if (!h || !out) return h ? lsm_fail(h, LSM_ERR_INVALID, f + "null argument") : LSM_ERR_INVALID;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (!phi && !given) return lsm_fail(h, LSM_ERR_INVALID, f + "give phi or the cell " + cells);
    const int N = h->grid.ndim;
    if (N == 1) return lsm_fail(h, LSM_ERR_INVALID, f + "a 1-dimensional grid is not supported (2-D and 3-D only)");
    if (h->comm) return lsm_fail(h, LSM_ERR_INVALID, f + "the handle has a communicator attached (single device only)");
    if (h->bc[N - 1][0].kind == LSM_BC_NONE || h->bc[N - 1][1].kind == LSM_BC_NONE)
        return lsm_fail(h, LSM_ERR_INVALID, f + "the handle is a slab of a multi-GPU grid (whole grids only)");
    for (int d = 0; d < N; ++d)
        if (h->nloc[d] < 3) return lsm_fail(h, LSM_ERR_INVALID, f + "at least 3 nodes (2 cells) per dimension");
    if (!given && (!(v_in > 0) || !std::isfinite(v_in) || !(v_out > 0) || !std::isfinite(v_out)))
        return lsm_fail(h, LSM_ERR_INVALID, f + in + " and " + outn + " must be finite and positive");
    if (!given && !std::isfinite(level)) return lsm_fail(h, LSM_ERR_INVALID, f + "level must be finite");
    return LSM_OK;
}
static int cp_check_precond(LsmHandle* h, const char* fn, int precond) {
    if (precond != LSM_PRECOND_MG && precond != LSM_PRECOND_JACOBI) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": unknown preconditioner");
    return LSM_OK;
}

// A x = f away from the pin by PCG from `guess` (device, comps·nn; NULL: zero); the solution is left in o.V.x
template <class Level>
static int cp_pcg(LsmHandle* h, CellProblem<Level>& o, const char* fn, const double* f, const double* guess, double rtol, int max_iters, int* iters, double* relres) {
    const int N = o.N;
    const Level& L = o.lev[0];
    const int jac = o.precond == LSM_PRECOND_JACOBI;
    hipStream_t st = h->stream;
    const int nt = (int)o.nt();
    const unsigned nb = mg_blocks(L.nn), nbt = mg_blocks(nt);
    const int r0 = mg_reset(h, o, rtol, max_iters, st);
    if (r0 != LSM_OK) return r0;
    hipLaunchKernelGGL(cp_start_kernel, dim3(nbt), dim3(MG_THREADS), 0, st, L.nn, nt, guess, o.V.x, o.V.p);
    MG_LAUNCH2(N, cp_init_kernel, Level, dim3(nb), MG_THREADS, st, L, o.V, (const double*)o.V.x, f, o.V.r, o.V.z, jac);
    LSM_HIP(h, hipGetLastError());
    const int r1 = mg_iterate(h, o, max_iters, st, [&](int) {
        if (!jac) mg_vcycle(o, o.V.r, st);
        hipLaunchKernelGGL(cp_dir_kernel, dim3(nbt), dim3(MG_THREADS), 0, st, nt, o.V);
        MG_LAUNCH2(N, cp_k1_kernel, Level, dim3(nb), MG_THREADS, st, L, (const double*)o.V.p, o.V.q, o.partial.p, o.st.p);
        if (jac) hipLaunchKernelGGL(mg_k2_kernel<1>, dim3(nbt), dim3(MG_THREADS), 0, st, L.D, nt, (MgVec)o.V, (const double*)o.V.p);
        else hipLaunchKernelGGL(mg_k2_kernel<0>, dim3(nbt), dim3(MG_THREADS), 0, st, L.D, nt, (MgVec)o.V, (const double*)o.V.p);
    });
    if (r1 != LSM_OK) return r1;
    return mg_report(h, o, fn, rtol, iters, relres);
}

static int cp_check_tol(LsmHandle* h, const char* fn, double rtol, int max_iters) {
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": rtol must be positive and max_iters at least 1");
    return LSM_OK;
}

// all K cell problems, one after the other; load(k) enqueues problem k's right-hand side into o.f.  The stored correctors change
// only when all K have converged
template <class Level, class Load>
static int cp_solve_all(LsmHandle* h, CellProblem<Level>& o, const char* fn, const double* chi_guess, double rtol, int max_iters, int* iters, double* relres, Load load) {
    const int rc = cp_check_tol(h, fn, rtol, max_iters);
    if (rc != LSM_OK) return rc;
    const int K = o.K;
    (void)hipSetDevice(h->device);
    hipStream_t st = h->stream;
    const size_t nt = o.nt();
    for (int k = 0; k < K; ++k) {
        if (iters) iters[k] = 0;
        if (relres) relres[k] = 0.0;
    }
    const double* guess = nullptr;
    if (chi_guess) {      // the caller's memory, host or device: staged where the new correctors will land
        LSM_HIP(h, hipMemcpyAsync(o.chinew, chi_guess, (size_t)K * nt * sizeof(double), hipMemcpyDefault, st));
        LSM_HIP(h, hipStreamSynchronize(st));
        guess = o.chinew;
    }
    for (int k = 0; k < K; ++k) {
        load(k);
        const int r = cp_pcg(h, o, fn, o.f, guess ? guess + k * nt : nullptr, rtol, max_iters, iters ? iters + k : nullptr, relres ? relres + k : nullptr);
        if (r != LSM_OK) return r;      // the stored correctors are untouched
        LSM_HIP(h, hipMemcpyAsync(o.chinew + k * nt, o.V.x, nt * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    LSM_HIP(h, hipMemcpyAsync(o.chi, o.chinew, (size_t)K * nt * sizeof(double), hipMemcpyDeviceToDevice, st));
    LSM_HIP(h, hipStreamSynchronize(st));
    return LSM_OK;
}

template <class Level>
static int cp_solve_rhs(LsmHandle* h, CellProblem<Level>& o, const char* fn, const double* f, double* x, double rtol, int max_iters, int* iters, double* relres) {
    if (!f || !x || f == x) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": f and x must be two arrays");
    const int rc = cp_check_tol(h, fn, rtol, max_iters);
    if (rc != LSM_OK) return rc;
    (void)hipSetDevice(h->device);
    const int r = cp_pcg(h, o, fn, f, x, rtol, max_iters, iters, relres);
    if (r != LSM_OK) return r;
    LSM_HIP(h, hipMemcpyAsync(x, o.V.x, o.nt() * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    LSM_HIP(h, hipStreamSynchronize(h->stream));
    return LSM_OK;
}

// the stored correctors from (to_device) or into the caller's memory, host or device
template <class Level>
static int cp_copy_correctors(LsmHandle* h, CellProblem<Level>& o, const char* fn, double* chi, bool to_device) {
    if (!chi) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": null argument");
    const size_t bytes = (size_t)o.K * o.nt() * sizeof(double);
    LSM_HIP(h, hipMemcpyAsync(to_device ? o.chi : chi, to_device ? chi : o.chi, bytes, hipMemcpyDefault, h->stream));
    LSM_HIP(h, hipStreamSynchronize(h->stream));
    return LSM_OK;
}
template <class Level>
static int cp_set_correctors(LsmHandle* h, CellProblem<Level>& o, const char* fn, const double* chi) { return cp_copy_correctors(h, o, fn, const_cast<double*>(chi), true); }
template <class Level>
static int cp_correctors(LsmHandle* h, CellProblem<Level>& o, const char* fn, double* chi_out) { return cp_copy_correctors(h, o, fn, chi_out, false); }

template <class Level>
static int cp_cells(LsmHandle* h, CellProblem<Level>& o, const char* fn, double* out) {
    if (!out) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": null argument");
    const Level& L = o.lev[0];
    LSM_HIP(h, hipMemcpyAsync(out, L.cell, (size_t)L.nn * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return LSM_OK;
}

// corrector k into the handle's fields U
template <class Level>
static int cp_store(LsmHandle* h, CellProblem<Level>& o, int k, CpFields U) {
    MG_LAUNCH2(o.N, cp_store_kernel, Level, dim3(mg_blocks(o.nnf())), MG_THREADS, h->stream, o.lev[0], o.G, o.F, (const double*)(o.chi + (size_t)k * o.nt()), U);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

// the K×K tensor: launch(0) enqueues the file's tensor kernel, which leaves the NP sums in o.sums; mirrored, over the cells' count
template <class Level, class Launch>
static int cp_tensor(LsmHandle* h, CellProblem<Level>& o, const char* fn, double* T, Launch launch) {
    if (!T) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": null argument");
    hipStream_t st = h->stream;
    launch(0);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipMemcpyAsync(o.h_sums.p, o.sums, o.NP * sizeof(double), hipMemcpyDeviceToHost, st));
    LSM_HIP(h, hipStreamSynchronize(st));
    const int K = o.K;
    for (int q = 0; q < K; ++q)
        for (int p = 0; p <= q; ++p) T[p * K + q] = T[q * K + p] = o.h_sums.p[q * (q + 1) / 2 + p] / (double)o.lev[0].nn;
    return LSM_OK;
}

// the sensitivity for the K×K weights W (host): launch(1) enqueues the tensor kernel without its reduction, which reads o.W and
// leaves a value per cell in o.cell; gathered to the handle's nodes
template <class Level, class Launch>
static int cp_sensitivity(LsmHandle* h, CellProblem<Level>& o, const char* fn, const double* W, void* g_out, Launch launch) {
    if (!W || !g_out) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": null argument");
    const int K = o.K;
    for (int p = 0; p < K; ++p)
        for (int q = 0; q < K; ++q)
            if (!std::isfinite(W[p * K + q]) || W[p * K + q] != W[q * K + p]) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": W must be finite and symmetric");
    hipStream_t st = h->stream;
    LSM_HIP(h, hipMemcpyAsync(o.W, W, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice, st));
    LSM_HIP(h, hipStreamSynchronize(st));      // W is the caller's pageable memory
    launch(1);
    MG_LAUNCH2(o.N, cp_sens_gather_kernel, Level, dim3(mg_blocks(o.nnf())), MG_THREADS, st, o.lev[0], o.G, o.F, (const double*)o.cell, g_out);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

}  // namespace lsm
