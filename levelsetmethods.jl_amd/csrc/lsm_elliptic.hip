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
// The PCG iteration and the V-cycle are mg_pcg.h's, with one component per node and ω = 0.8.  What is this file's own:
//   K1  p' = z + β p fused into the apply (p double-buffered: neighbours read the old one),  q = A p',  σ = p'·q   → α = ρ/σ
//   a NULL mask (no fixed node) costs no read; a neighbour's mask byte is read instead of its value where it is fixed.
// The batched solve (lsm_elliptic_solve_many) is mg_pcg.h's batched V-cycle and K2 with this file's init (a MANY switch)
// and store: the column is blockIdx.z, its vectors lie at the column stride nn, its fields come as K pointers in a kernel argument.  Its
// K1 (el_k1_many_kernel) keeps the columns in one workgroup instead: a thread owns a node for all columns and forms its coefficients once.
#include "el_cell.h"
#include "lobpcg.h"
#include "mg_pcg.h"

namespace lsm {

static const double EL_OMEGA = 0.8;
enum { EL_BAD_PHI = 0, EL_BAD_A = 1, EL_BAD_C = 2, EL_NFIXED = 3, EL_CPOS = 4, EL_NSTAT = 8 };

struct ElVec : MgVec { double* p[2]; };     // p double-buffered: K1 writes the one, its neighbours read the other
struct ElUMany { void* p[MG_MAXCOLS]; };    // the fields of the columns of a batched call
struct ElW { double w[MG_MAXCOLS]; };       // their weights

struct ElLevel {
    int n[3];
    int nn;
    double h[3], ih2[3];
    const double* a;              // cells, n−1 per axis
    const double* cn;             // c per node, or NULL: cc everywhere
    double cc;
    const unsigned char* mask;    // one byte per node, or NULL: no fixed node
    const double* D;              // the diagonal

    using Vec = ElVec;
    static constexpr int comps(int) { return 1; }
    __device__ __forceinline__ bool fixed(int id, int) const { return mask && mask[id]; }
    __device__ __forceinline__ static double omega() { return EL_OMEGA; }
    static void launch_resid(int N, unsigned nb, hipStream_t s, const ElLevel& L, const double* r, const double* x, double* res, const MgState* st);
    static void launch_resid_many(int N, unsigned nb, unsigned cols, hipStream_t s, const ElLevel& L, const double* r, const double* x, double* res,
                                  const MgState* st);
    // the eliminated operator at a free node: with MASK fixed neighbours count as zero unread, without it x holds zero there
    template <int N, bool MASK>
    __device__ __forceinline__ void apply(int id, const int I[3], const double* x, int stride, double out[1]) const;
};

// the 2^N cells around node I: bit d of m set: cell index I_d along d, clear: I_d − 1; zero where there is no cell
template <int N>
__device__ __forceinline__ void el_cells_around(const ElLevel& L, const int I[3], double v[1 << N]) {
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {
        int C[3] = {0, 0, 0};
        bool in = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            C[d] = I[d] - 1 + ((m >> d) & 1);
            in = in && C[d] >= 0 && C[d] < L.n[d] - 1;
        }
        v[m] = in ? L.a[mg_cell_index<N>(L.n, C)] : 0.0;
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
__device__ __forceinline__ double el_cm(const ElLevel& L, int id, const int I[3]) { return (L.cn ? L.cn[id] : L.cc) * mg_mass<N>(L.n, I); }

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
template <int N, bool MASK>
__device__ __forceinline__ void ElLevel::apply(int id, const int I[3], const double* x, int, double out[1]) const {
    out[0] = el_apply<N>(*this, id, I, x[id], [&](int q) { return MASK && fixed(q, 0) ? 0.0 : x[q]; });
}

// ---- setup of level 0: the cell array from ϕ (or the caller's, checked), c checked, fixed nodes counted.  One thread per node;
// a node that is the lowest corner of a cell writes that cell.
template <int N>
__global__ void __launch_bounds__(MG_THREADS) el_setup_kernel(ElLevel L, MgField F, const void* __restrict__ phi, double level, double a_in, double a_out,
                                                              double hmin, const double* __restrict__ a_given, double* __restrict__ a, unsigned long long* st) {
    unsigned cnt[5] = {0, 0, 0, 0, 0};      // per thread, added once per wave: one atomic per node on one word serialises the launch
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        if (phi && !mg_finite(ld_val(phi, mg_padded(F, I), F.f32))) ++cnt[EL_BAD_PHI];
        const double c = L.cn ? L.cn[id] : L.cc;
        if (!(c >= 0.0) || !mg_finite(c)) ++cnt[EL_BAD_C];
        else if (c > 0.0) ++cnt[EL_CPOS];
        if (L.fixed(id, 0)) ++cnt[EL_NFIXED];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && I[d] < L.n[d] - 1;
        if (!corner) continue;
        const int ci = I[0] + (L.n[0] - 1) * (I[1] + (N > 2 ? (L.n[1] - 1) * I[2] : 0));
        double av;
        if (a_given) {
            av = a_given[ci];
            if (!(av > 0.0) || !mg_finite(av)) ++cnt[EL_BAD_A];
        } else {
            av = el_cell_from_phi<N>(phi, mg_padded(F, I), F.s1, F.s2, F.f32, level, a_in, a_out, hmin);
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
__global__ void __launch_bounds__(MG_THREADS) el_coarsen_kernel(ElLevel Lf, ElLevel Lc, int co0, int co1, int co2, double* __restrict__ ac,
                                                                double* __restrict__ cnc, unsigned char* __restrict__ fixc) {
    const int co[3] = {co0, co1, co2};
    const double scale = mg_coarsen_scale(co0 + co1 + co2);
    MG_LOOP(id, Lc.nn) {
        int J[3];
        mg_coords<N>(Lc.n, id, J);
        const int fid = (co[0] ? 2 * J[0] : J[0]) + Lf.n[0] * ((co[1] ? 2 * J[1] : J[1]) + (N > 2 ? Lf.n[1] * (co[2] ? 2 * J[2] : J[2]) : 0));
        if (cnc) cnc[id] = Lf.cn[fid];
        if (fixc) fixc[id] = Lf.mask[fid];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && J[d] < Lc.n[d] - 1;
        if (!corner) continue;
        ac[mg_cell_index<N>(Lc.n, J)] = mg_cell_average<N>(Lf.a, Lf.n, J, co, scale);
    }
}

// ---- the diagonal of a level
template <int N>
__global__ void __launch_bounds__(MG_THREADS) el_diag_kernel(ElLevel L, double* __restrict__ D) {
    const double half = N == 2 ? 0.5 : 0.25;
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
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
__global__ void __launch_bounds__(MG_THREADS) el_apply_kernel(ElLevel L, const double* __restrict__ x, double* __restrict__ y) {
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        y[id] = el_apply<N>(L, id, I, x[id], [&](int q) { return x[q]; });
    }
}

// ---- the energy density e_I = Σ_d (Σ_± k̄·(g·g), g = (u_J − u_I)/h_d)/(existing edges along d at I), into a field of the handle
template <int N>
__global__ void __launch_bounds__(MG_THREADS) el_energy_kernel(ElLevel L, MgField F, const void* __restrict__ u, void* __restrict__ e_out) {
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double v[1 << N];
        el_cells_around<N>(L, I, v);
        const long long at = mg_padded(F, I);
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
__global__ void __launch_bounds__(MG_THREADS) el_compliance_kernel(ElLevel L, MgField F, const double* __restrict__ f, const void* __restrict__ u,
                                                                   double* partial, MgState* st) {
    double red[1] = {0.0};
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        red[0] += (mg_mass<N>(L.n, I) * f[id]) * ld_val(u, mg_padded(F, I), F.f32);
    }
    if (!block_reduce_ordered<1, MG_THREADS>(red, partial, &st->ticket[3]) || threadIdx.x != 0) return;
    st->out = red[0];
}

// ---- PCG
// x₀ = u (the guess and the Dirichlet values), b = m·f, r₀ = b − A x₀ on the free nodes, 0 on the fixed ones; ‖b_free‖², ‖r₀‖²;
// jac: z = r/D and ρ = r·z as well.  MANY: column blockIdx.z of a batch; its field is um.p[blockIdx.z] (um: one ElUMany; u is not read)
template <int N, int MANY = 0, class... UM>
__global__ void __launch_bounds__(MG_THREADS) el_init_kernel(ElLevel L, MgField F, ElVec V, const double* __restrict__ f, const void* __restrict__ u, int jac,
                                                             UM... um) {
    if constexpr (MANY) {
        const size_t c = blockIdx.z, at = c * (size_t)L.nn;
        V.x += at; V.r += at; V.z += at; V.p[0] += at; f += at;
        V.partial += c * (4 * MG_MAXB);
        V.st += c;
        u = (um.p[c], ...);
    }
    double red[4] = {0.0, 0.0, 0.0, 0.0};     // ‖b_free‖², ‖r₀‖², r·z, non-finite entries (a count below 2^53: exact)
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
        const long long fs[3] = {1, F.s1, F.s2};
        const int cs[3] = {1, L.n[0], L.n[0] * L.n[1]};
        const double ui = ld_val(u, at, F.f32), fi = f[id];
        if (!mg_finite(ui) || !mg_finite(fi)) red[3] += 1.0;
        double r = 0.0, z = 0.0;
        if (!L.fixed(id, 0)) {
            const double b = mg_mass<N>(L.n, I) * fi;
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
    if (!block_reduce_ordered<4, MG_THREADS>(red, V.partial, &V.st->ticket[0]) || threadIdx.x != 0) return;
    mg_init_tail(*V.st, red, jac);
}

// K1: p' = z + β p, q = A p' (eliminated), σ = p'·q, α = ρ/σ
template <int N>
__global__ void __launch_bounds__(MG_THREADS) el_k1_kernel(ElLevel L, ElVec V, int par) {
    if (V.st->status != MG_RUN) return;
    const double beta = V.st->beta;
    const double* __restrict__ z = V.z;
    const double* __restrict__ po = V.p[par];
    double* __restrict__ pn = V.p[par ^ 1];
    double red[1] = {0.0};
    MG_LOOP(id, L.nn) {
        double pp = 0.0, q = 0.0;
        if (!L.fixed(id, 0)) {
            int I[3];
            mg_coords<N>(L.n, id, I);
            pp = z[id] + beta * po[id];
            q = el_apply<N>(L, id, I, pp, [&](int j) { return L.fixed(j, 0) ? 0.0 : z[j] + beta * po[j]; });
            red[0] += pp * q;
        }
        pn[id] = pp;
        V.q[id] = q;
    }
    if (!block_reduce_ordered<1, MG_THREADS>(red, V.partial, &V.st->ticket[1]) || threadIdx.x != 0) return;
    mg_k1_tail(*V.st, red[0]);
}

// K1 of a batch of NCOL columns (vectors at the column stride nn, states and partials per column, as mg_pcg.h lays a batch out).  The
// columns are not on blockIdx.z here: a thread owns a node for all of them — the cells, the edge coefficients, c·m and the neighbours'
// mask bytes once, as elm_apply_kernel forms them (in the scalar operator they are most of an apply), then per running column
// el_k1_kernel's arithmetic in its order; a column that has left MG_RUN is skipped.  The launch shape and the grid-stride assignment of
// nodes to threads are el_k1_kernel's, and p'·q is reduced per column into that column's own partials and ticket: the same partials in
// the same order, hence the single solve's bits.  NCOL is a compile-time count, so that red[] stays in registers; the z-column form of
// this kernel (a MANY switch on el_k1_kernel) was built, measured slower and removed
template <int N, int NCOL>
__global__ void __launch_bounds__(MG_THREADS) el_k1_many_kernel(ElLevel L, ElVec V, int par) {
    bool run[NCOL], any = false;
    double beta[NCOL], red[NCOL];
#pragma unroll
    for (int k = 0; k < NCOL; ++k) {
        run[k] = V.st[k].status == MG_RUN;
        beta[k] = V.st[k].beta;
        red[k] = 0.0;
        any = any || run[k];
    }
    if (!any) return;
    const double* __restrict__ z = V.z;
    const double* __restrict__ po = V.p[par];
    double* __restrict__ pn = V.p[par ^ 1];
    double* __restrict__ qv = V.q;
    const int cs[3] = {1, L.n[0], L.n[0] * L.n[1]};
    const double half = N == 2 ? 0.5 : 0.25;
    const size_t nn = (size_t)L.nn;
    MG_LOOP(id, L.nn) {
        if (L.fixed(id, 0)) {
#pragma unroll
            for (int k = 0; k < NCOL; ++k)
                if (run[k]) {
                    pn[k * nn + id] = 0.0;
                    qv[k * nn + id] = 0.0;
                }
            continue;
        }
        int I[3];
        mg_coords<N>(L.n, id, I);
        double v[1 << N];
        el_cells_around<N>(L, I, v);
        double w[2 * N];
        int q[2 * N];
        bool edge[2 * N], rd[2 * N];      // the edge exists; its far node is free (its value is read)
#pragma unroll
        for (int d = 0; d < N; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int e = 2 * d + s;
                edge[e] = s ? I[d] < L.n[d] - 1 : I[d] > 0;
                q[e] = edge[e] ? (s ? id + cs[d] : id - cs[d]) : id;
                rd[e] = edge[e] && !L.fixed(q[e], 0);
                w[e] = (el_edge_sum<N>(v, d, s) * half) * L.ih2[d];
            }
        const double cm = el_cm<N>(L, id, I);
#pragma unroll
        for (int k = 0; k < NCOL; ++k) {
            if (!run[k]) continue;
            const double* __restrict__ zk = z + k * nn;
            const double* __restrict__ pk = po + k * nn;
            const double pp = zk[id] + beta[k] * pk[id];
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < 2 * N; ++e) {
                const double xn = rd[e] ? zk[q[e]] + beta[k] * pk[q[e]] : 0.0;
                if (edge[e]) acc = acc + w[e] * (pp - xn);
            }
            const double qq = acc + cm * pp;
            red[k] += pp * qq;
            pn[k * nn + id] = pp;
            qv[k * nn + id] = qq;
        }
    }
#pragma unroll
    for (int k = 0; k < NCOL; ++k) {
        if (!run[k]) continue;      // uniform over the grid
        double r1[1] = {red[k]};
        if (block_reduce_ordered<1, MG_THREADS>(r1, V.partial + (size_t)k * (4 * MG_MAXB), &V.st[k].ticket[1]) && threadIdx.x == 0) mg_k1_tail(V.st[k], r1[0]);
        __syncthreads();      // the reduction's LDS is reused by the next column
    }
}

// ---- x → u on the free nodes (rounded to the storage type); the fixed nodes and the ghosts are left as they are
template <int N>
__global__ void __launch_bounds__(MG_THREADS) el_store_kernel(ElLevel L, MgField F, const double* __restrict__ x, void* __restrict__ u) {
    MG_LOOP(id, L.nn) {
        if (L.fixed(id, 0)) continue;
        int I[3];
        mg_coords<N>(L.n, id, I);
        st_val(u, mg_padded(F, I), F.f32, x[id]);
    }
}

// the same for the columns of a batch: column blockIdx.z of x into its field
template <int N>
__global__ void __launch_bounds__(MG_THREADS) el_store_many_kernel(ElLevel L, MgField F, const double* __restrict__ x, ElUMany U) {
    x += (size_t)blockIdx.z * L.nn;
    void* __restrict__ u = U.p[blockIdx.z];
    MG_LOOP(id, L.nn) {
        if (L.fixed(id, 0)) continue;
        int I[3];
        mg_coords<N>(L.n, id, I);
        st_val(u, mg_padded(F, I), F.f32, x[id]);
    }
}

// ---- the fields of a batch
// what el_energy_kernel forms at a node before it reads u: per edge k̄ = S/(cells of the edge) and whether the edge exists
template <int N>
struct ElEdges {
    double kb[2 * N];
    bool on[2 * N];
    long long off[2 * N];
};
template <int N>
__device__ __forceinline__ void el_edges(const ElLevel& L, const MgField& F, const int I[3], ElEdges<N>& E) {
    double v[1 << N];
    el_cells_around<N>(L, I, v);
    const long long fs[3] = {1, F.s1, F.s2};
#pragma unroll
    for (int d = 0; d < N; ++d) {
        double ncell = 1.0;
#pragma unroll
        for (int o = 0; o < N; ++o)
            if (o != d && I[o] > 0 && I[o] < L.n[o] - 1) ncell = ncell * 2.0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            E.on[2 * d + s] = s ? I[d] < L.n[d] - 1 : I[d] > 0;
            E.kb[2 * d + s] = el_edge_sum<N>(v, d, s) / ncell;
            E.off[2 * d + s] = s ? fs[d] : -fs[d];
        }
    }
}
// el_energy_kernel's sums at a node with g·g replaced by g_u·g_v (v = u: its bits)
template <int N>
__device__ __forceinline__ double el_energy_at(const ElLevel& L, const MgField& F, const ElEdges<N>& E, long long at, const void* __restrict__ u,
                                               const void* __restrict__ v) {
    const double ui = ld_val(u, at, F.f32), vi = ld_val(v, at, F.f32);
    double e = 0.0;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        double s = 0.0, cnt = 0.0;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int k = 2 * d + side;
            if (E.on[k]) {
                const double gu = (ld_val(u, at + E.off[k], F.f32) - ui) / L.h[d];
                const double gv = (ld_val(v, at + E.off[k], F.f32) - vi) / L.h[d];
                s = s + E.kb[k] * (gu * gv);
                cnt = cnt + 1.0;
            }
        }
        e = e + s / cnt;
    }
    return e;
}
// ---- the mutual energy density m_I(u, v): the a∇u·∇v part only (the c·u·v term is not in it, as it is not in el_energy_kernel)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) el_energy_mutual_kernel(ElLevel L, MgField F, const void* __restrict__ u, const void* __restrict__ v,
                                                                      void* __restrict__ e_out) {
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        ElEdges<N> E;
        el_edges<N>(L, F, I, E);
        const long long at = mg_padded(F, I);
        st_val(e_out, at, F.f32, el_energy_at<N>(L, F, E, at, u, v));
    }
}
// ---- the weighted energy density of ncol columns in one pass: e_I = Σ_k w_k·e_{k,I}, k ascending from +0, e_{k,I} el_energy_kernel's
// value of column k in fp64.  The edge coefficients and the counts of a node once; inside, the columns, each e_k finished before
// w_k·e_k is added (no accumulator per column: nothing is indexed by k but the kernel arguments)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) el_energy_many_kernel(ElLevel L, MgField F, ElUMany U, int ncol, ElW W, void* __restrict__ e_out) {
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        ElEdges<N> E;
        el_edges<N>(L, F, I, E);
        const long long at = mg_padded(F, I);
        double e = 0.0;
#pragma unroll 1
        for (int k = 0; k < ncol; ++k) e = e + W.w[k] * el_energy_at<N>(L, F, E, at, U.p[k], U.p[k]);
        st_val(e_out, at, F.f32, e);
    }
}

// ---- host side
void ElLevel::launch_resid(int N, unsigned nb, hipStream_t s, const ElLevel& L, const double* r, const double* x, double* res, const MgState* st) {
    MG_LAUNCH2(N, mg_resid_kernel, ElLevel, nb, MG_THREADS, s, L, r, x, res, st);
}
void ElLevel::launch_resid_many(int N, unsigned nb, unsigned cols, hipStream_t s, const ElLevel& L, const double* r, const double* x, double* res,
                                const MgState* st) {
    MG_LAUNCH3(N, mg_resid_kernel, ElLevel, 1, dim3(nb, 1, cols), MG_THREADS, s, L, r, x, res, st);
}
struct EllipticObject : MgSolver<ElLevel> {
    // the batched solve's workspace: the vectors, states and partials of `cols` columns, with the levels (cells, D, c, masks) shared.
    // Made by the first lsm_elliptic_solve_many, grown when a later one asks for more columns; the single solve's workspace, which
    // the modes borrow, is not touched
    std::unique_ptr<MgSolver<ElLevel>> many;
};

}  // namespace lsm

using namespace lsm;

struct LsmElliptic { LsmHandle* h; EllipticObject* o; };

static int el_create(LsmHandle* h, EllipticObject& o, const void* phi, double level, double a_in, double a_out, const double* a_cells, double c_const,
                     const double* c_nodes, const unsigned char* fixed, int64_t stats[4]) {
    const int N = h->grid.ndim;
    o.N = N;
    o.F = MgField{h->lay.stride[1], N > 2 ? h->lay.stride[2] : 0, h->lay.origin, h->dtype == LSM_DTYPE_F32 ? 1 : 0};
    std::vector<ElLevel> lev;
    ElLevel L;
    memset(&L, 0, sizeof(L));
    L.cc = c_const;
    double hmin;
    const long long nn = mg_shapes(h, L, 1LL << 29, lev, o.co, hmin);
    if (lev.empty()) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: the grid is too large (2^29 nodes at most)");
    for (ElLevel& q : lev)
        for (int d = 0; d < 3; ++d) q.ih2[d] = 1.0 / (q.h[d] * q.h[d]);
    const int nl = (int)lev.size();
    if (lev[nl - 1].nn > 128) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_create: the coarsest level has more than 128 nodes");
    // one allocation of doubles: per level cells, D, [c], xa, xb, [rhs]; level 0: x r q p0 p1 as well
    size_t nd = 0, nb = 0;
    for (int l = 0; l < nl; ++l) {
        nd += mg_ncells(N, lev[l]) + (size_t)lev[l].nn * (size_t)(3 + (c_nodes ? 1 : 0) + (l ? 1 : 5));
        nb += (size_t)lev[l].nn;
    }
    LSM_HIP(h, o.buf.alloc(nd * sizeof(double)));
    if (fixed) LSM_HIP(h, o.fx.alloc(nb));
    hipStream_t s = h->stream;
    const int ra = mg_alloc_scalars(h, o, EL_NSTAT, s);
    if (ra != LSM_OK) return ra;
    double* b = o.buf;
    unsigned char* fb = o.fx;
    std::vector<double*> acell(nl), dg(nl), cn(nl, nullptr);
    std::vector<unsigned char*> fxl(nl, nullptr);
    o.rhs.assign(nl, nullptr); o.xa.assign(nl, nullptr); o.xb.assign(nl, nullptr);
    for (int l = 0; l < nl; ++l) {
        const size_t m = (size_t)lev[l].nn;
        acell[l] = b; b += mg_ncells(N, lev[l]);
        dg[l] = b; b += m;
        if (c_nodes) { cn[l] = b; b += m; }
        o.xa[l] = b; b += m;
        o.xb[l] = b; b += m;
        if (l) { o.rhs[l] = b; b += m; }
        else {
            o.V.x = b; b += m; o.V.r = b; b += m; o.V.q = b; b += m; o.V.p[0] = b; b += m; o.V.p[1] = b; b += m;
        }
        if (fixed) { fxl[l] = fb; fb += m; }
        lev[l].a = acell[l]; lev[l].D = dg[l]; lev[l].cn = cn[l]; lev[l].mask = fxl[l];
    }
    if (c_nodes) LSM_HIP(h, hipMemcpyAsync(cn[0], c_nodes, (size_t)nn * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (fixed) LSM_HIP(h, hipMemcpyAsync(fxl[0], fixed, (size_t)nn, hipMemcpyDeviceToDevice, s));
    MG_LAUNCH(N, el_setup_kernel, mg_blocks(nn), MG_THREADS, s, lev[0], o.F, a_cells ? (const void*)nullptr : phi, level, a_in, a_out, hmin, a_cells,
              acell[0], o.cnt.p);
    LSM_HIP(h, hipGetLastError());
    unsigned long long c[EL_NSTAT] = {};
    LSM_HIP(h, hipMemcpyAsync(c, o.cnt.p, sizeof(c), hipMemcpyDeviceToHost, s));
    LSM_HIP(h, hipStreamSynchronize(s));
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
        MG_LAUNCH(N, el_coarsen_kernel, mg_blocks(lev[l].nn), MG_THREADS, s, lev[l - 1], lev[l], o.co[l - 1][0], o.co[l - 1][1], o.co[l - 1][2], acell[l], cn[l],
                  fxl[l]);
    for (int l = 0; l < nl; ++l) MG_LAUNCH(N, el_diag_kernel, mg_blocks(lev[l].nn), MG_THREADS, s, lev[l], dg[l]);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(s));
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
    MG_LAUNCH(s->o->N, el_apply_kernel, mg_blocks(L.nn), MG_THREADS, s->h->stream, L, x, y);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elliptic_cells(LsmElliptic* s, double* a_out_cells) {
    if (!s) return LSM_ERR_INVALID;
    if (!a_out_cells) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_cells: null argument");
    const ElLevel& L = s->o->lev[0];
    const size_t m = mg_ncells(s->o->N, L);
    LSM_HIP(s->h, hipMemcpyAsync(a_out_cells, L.a, m * sizeof(double), hipMemcpyDeviceToDevice, s->h->stream));
    return LSM_OK;
}

int lsm_elliptic_energy(LsmElliptic* s, const void* u, void* e_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!u || !e_out || u == e_out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_energy: u and e_out must be two fields");
    const ElLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, el_energy_kernel, mg_blocks(L.nn), MG_THREADS, s->h->stream, L, s->o->F, u, e_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elliptic_compliance(LsmElliptic* s, const double* f, const void* u, double* out) {
    if (!s) return LSM_ERR_INVALID;
    if (!f || !u || !out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_compliance: null argument");
    EllipticObject& o = *s->o;
    const ElLevel& L = o.lev[0];
    hipStream_t st = s->h->stream;
    MG_LAUNCH(o.N, el_compliance_kernel, mg_blocks(L.nn), MG_THREADS, st, L, o.F, f, u, o.partial.p, o.st.p);
    LSM_HIP(s->h, hipGetLastError());
    LSM_HIP(s->h, hipMemcpyAsync(o.h_st, o.st, sizeof(MgState), hipMemcpyDeviceToHost, st));
    LSM_HIP(s->h, hipStreamSynchronize(st));
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
    const int r0 = mg_reset(h, o, rtol, max_iters, st);
    if (r0 != LSM_OK) return r0;
    const unsigned nb = mg_blocks(L.nn);
    MG_LAUNCH(N, el_init_kernel, nb, MG_THREADS, st, L, o.F, o.V, f, (const void*)u, jac);
    LSM_HIP(h, hipGetLastError());
    const int r1 = mg_iterate(h, o, max_iters, st, [&](int enq) {
        const int par = enq & 1;
        if (!jac) mg_vcycle(o, o.V.r, st);
        MG_LAUNCH(N, el_k1_kernel, nb, MG_THREADS, st, L, o.V, par);
        if (jac) hipLaunchKernelGGL(mg_k2_kernel<1>, dim3(nb), dim3(MG_THREADS), 0, st, L.D, L.nn, (MgVec)o.V, (const double*)o.V.p[par ^ 1]);
        else hipLaunchKernelGGL(mg_k2_kernel<0>, dim3(nb), dim3(MG_THREADS), 0, st, L.D, L.nn, (MgVec)o.V, (const double*)o.V.p[par ^ 1]);
    });
    if (r1 != LSM_OK) return r1;
    const int r2 = mg_report(h, o, "lsm_elliptic_solve", rtol, iters_out, relres_out);
    if (r2 != LSM_OK) return r2;
    MG_LAUNCH(N, el_store_kernel, nb, MG_THREADS, st, L, o.F, (const double*)o.V.x, u);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(st));
    return LSM_OK;
}

// the batch workspace for K columns.  A larger one is built beside the old and takes its place only when every allocation succeeded
static int el_many_reserve(LsmHandle* h, EllipticObject& o, int K) {
    if (o.many && o.many->cols >= K) return LSM_OK;
    std::unique_ptr<MgSolver<ElLevel>> w(new MgSolver<ElLevel>());
    MgSolver<ElLevel>& M = *w;
    const int nl = (int)o.lev.size();
    M.N = o.N; M.precond = o.precond; M.cols = K; M.F = o.F;
    M.lev = o.lev;
    memcpy(M.co, o.co, sizeof(M.co));
    // per level xa, xb, [rhs]; level 0: x r q p0 p1 as well
    size_t nd = 0;
    for (int l = 0; l < nl; ++l) nd += (size_t)K * (size_t)o.lev[l].nn * (size_t)(l ? 3 : 7);
    LSM_HIP(h, M.buf.alloc(nd * sizeof(double)));
    LSM_HIP(h, M.partial.alloc((size_t)K * 4 * MG_MAXB * sizeof(double)));
    LSM_HIP(h, M.st.alloc(K * sizeof(MgState)));
    LSM_HIP(h, M.h_st.alloc(K * sizeof(MgState)));
    M.rhs.assign(nl, nullptr); M.xa.assign(nl, nullptr); M.xb.assign(nl, nullptr);
    double* b = M.buf;
    for (int l = 0; l < nl; ++l) {
        const size_t m = (size_t)K * (size_t)o.lev[l].nn;
        M.xa[l] = b; b += m;
        M.xb[l] = b; b += m;
        if (l) { M.rhs[l] = b; b += m; }
        else {
            M.V.x = b; b += m; M.V.r = b; b += m; M.V.q = b; b += m; M.V.p[0] = b; b += m; M.V.p[1] = b; b += m;
        }
    }
    M.V.z = o.precond == LSM_PRECOND_JACOBI ? M.xa[0] : M.xb[0];
    M.V.partial = M.partial;
    M.V.st = M.st;
    o.many = std::move(w);
    return LSM_OK;
}

// K1 of a batch: el_k1_many_kernel for the handle's N and the K columns of the call (a compile-time count)
template <int N>
static void el_k1_many_launch(int K, unsigned nb, hipStream_t st, const ElLevel& L, const ElVec& V, int par) {
    switch (K) {
#define EL_K1_MANY_CASE(C) case C: hipLaunchKernelGGL((el_k1_many_kernel<N, C>), dim3(nb), dim3(MG_THREADS), 0, st, L, V, par); break;
        EL_K1_MANY_CASE(1) EL_K1_MANY_CASE(2) EL_K1_MANY_CASE(3) EL_K1_MANY_CASE(4) EL_K1_MANY_CASE(5) EL_K1_MANY_CASE(6) EL_K1_MANY_CASE(7) EL_K1_MANY_CASE(8)
#undef EL_K1_MANY_CASE
    }
}
static_assert(MG_MAXCOLS == 8 && LSM_ELLIPTIC_MAXCOLS == MG_MAXCOLS, "el_k1_many_launch has a case per column count");

// the K fields of a batched call: all given, no two the same
static bool el_fields_many(int K, void* const* u, ElUMany& U) {
    memset(&U, 0, sizeof(U));
    if (!u) return false;
    for (int a = 0; a < K; ++a) {
        if (!u[a]) return false;
        for (int b = 0; b < a; ++b)
            if (u[b] == u[a]) return false;
        U.p[a] = u[a];
    }
    return true;
}

int lsm_elliptic_solve_many(LsmElliptic* s, int K, const double* f, void* const* u, double rtol, int max_iters, int* iters, double* relres, int* status,
                            void* stream) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    EllipticObject& o = *s->o;
    ElUMany U;
    if (K < 1 || K > LSM_ELLIPTIC_MAXCOLS) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_solve_many: K must be 1 ... LSM_ELLIPTIC_MAXCOLS (8)");
    if (!f || !iters || !relres || !status || !el_fields_many(K, u, U))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_solve_many: f, the K distinct fields of u and the three result arrays must be given");
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_solve_many: rtol must be positive and max_iters at least 1");
    const int N = o.N;
    const ElLevel& L = o.lev[0];
    const int jac = o.precond == LSM_PRECOND_JACOBI;
    (void)hipSetDevice(h->device);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const int ra = el_many_reserve(h, o, K);
    if (ra != LSM_OK) return ra;
    MgSolver<ElLevel>& M = *o.many;
    const int r0 = mg_reset(h, M, rtol, max_iters, st, K);
    if (r0 != LSM_OK) return r0;
    const unsigned nb = mg_blocks(L.nn), nz = (unsigned)K;
    MG_LAUNCH3(N, el_init_kernel, 1, ElUMany, dim3(nb, 1, nz), MG_THREADS, st, L, o.F, M.V, f, (const void*)nullptr, jac, U);
    LSM_HIP(h, hipGetLastError());
    const int r1 = mg_iterate(h, M, max_iters, st, [&](int enq) {
        const int par = enq & 1;
        if (!jac) mg_vcycle<1>(M, M.V.r, st, K);
        if (N == 2) el_k1_many_launch<2>(K, nb, st, L, M.V, par);
        else el_k1_many_launch<3>(K, nb, st, L, M.V, par);
        if (jac) hipLaunchKernelGGL((mg_k2_kernel<1, 1>), dim3(nb, 1, nz), dim3(MG_THREADS), 0, st, L.D, L.nn, (MgVec)M.V, (const double*)M.V.p[par ^ 1]);
        else hipLaunchKernelGGL((mg_k2_kernel<0, 1>), dim3(nb, 1, nz), dim3(MG_THREADS), 0, st, L.D, L.nn, (MgVec)M.V, (const double*)M.V.p[par ^ 1]);
    }, K);
    if (r1 != LSM_OK) return r1;
    // every column's outcome; the error is that of the lowest column with non-finite input, else of the lowest that did not converge
    int bad = -1, bad_input = -1;
    for (int k = 0; k < K; ++k) {
        const MgState& S = M.h_st.p[k];
        iters[k] = S.iters;
        relres[k] = mg_relres(S);
        status[k] = S.status == MG_RUN ? (int)MG_MAXITER : S.status;
        if (S.status == MG_BREAK_INPUT && bad_input < 0) bad_input = k;
        if (S.status != MG_CONVERGED && bad < 0) bad = k;
    }
    if (bad >= 0) return mg_report(h, M, "lsm_elliptic_solve_many", rtol, nullptr, nullptr, bad_input >= 0 ? bad_input : bad);
    M.last_iters = 0;
    for (int k = 0; k < K; ++k) M.last_iters = std::max(M.last_iters, iters[k]);
    MG_LAUNCH(N, el_store_many_kernel, dim3(nb, 1, nz), MG_THREADS, st, L, o.F, (const double*)M.V.x, U);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(st));
    return LSM_OK;
}

int lsm_elliptic_energy_many(LsmElliptic* s, int K, void* const* u, const double* w, void* e_out) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    ElUMany U;
    ElW W;
    memset(&W, 0, sizeof(W));
    if (K < 1 || K > LSM_ELLIPTIC_MAXCOLS) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_energy_many: K must be 1 ... LSM_ELLIPTIC_MAXCOLS (8)");
    if (!w || !e_out || !el_fields_many(K, u, U)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_energy_many: the K distinct fields of u, w and e_out must be given");
    for (int k = 0; k < K; ++k) {
        if (u[k] == e_out) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_energy_many: e_out must not be one of the inputs");
        if (!std::isfinite(w[k])) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_energy_many: the weights must be finite");
        W.w[k] = w[k];
    }
    const ElLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, el_energy_many_kernel, mg_blocks(L.nn), MG_THREADS, h->stream, L, s->o->F, U, K, W, e_out);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

int lsm_elliptic_energy_mutual(LsmElliptic* s, const void* u, const void* v, void* e_out) {
    if (!s) return LSM_ERR_INVALID;
    if (!u || !v || !e_out) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_energy_mutual: u, v and e_out must be given");
    if (e_out == u || e_out == v) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elliptic_energy_mutual: e_out must not be one of the inputs");
    const ElLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, el_energy_mutual_kernel, mg_blocks(L.nn), MG_THREADS, s->h->stream, L, s->o->F, u, v, e_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

void lsm_elliptic_destroy(LsmElliptic* s) {
    if (!s) return;
    delete s->o;
    delete s;
}

// ======================================================================================================================================
// elliptic_modes: the m ≤ 8 smallest eigenpairs of A x = λ M x on the free nodes — A the operator above with its c term, the fixed nodes
// eliminated, M the lumped mass of an ersatz density — by lobpcg.h's LOBPCG, preconditioned by mg_vcycle (or 1/D).  include/lsm.h
// ("elliptic_modes") is the normative text, tests/_emodes_ref.py restates it, DESIGN.md §7.26 has the compiler's report.
//
// The iteration, its block passes and the workspace are lobpcg.h's with one component per node.  This file's own: the block apply, which
// loads a node's 2^N cells and forms its 2N edge coefficients once for all columns (in the scalar operator they are most of an apply's
// work), the stored mode and the sensitivity.  Nothing above this line changes: the modes object borrows the LsmElliptic's hierarchy, its
// xa / xb scratch, its MgState and its diagonal, and lsm_elliptic_solve resets the state it reads.
namespace lsm {

// ---- y_k = A x_k for ncols columns of nn doubles, the rows of fixed nodes zero, fixed neighbours read as zero.  A thread owns a node:
// the cells, the edge coefficients, c·m and the neighbours' mask bytes once, then per column el_apply's arithmetic in its order
template <int N>
__global__ void __launch_bounds__(MG_THREADS) elm_apply_kernel(ElLevel L, int ncols, const double* __restrict__ x, double* __restrict__ y) {
    const int cs[3] = {1, L.n[0], L.n[0] * L.n[1]};
    const double half = N == 2 ? 0.5 : 0.25;
    const size_t nn = (size_t)L.nn;
    MG_LOOP(id, L.nn) {
        if (L.fixed(id, 0)) {
            for (int k = 0; k < ncols; ++k) y[k * nn + id] = 0.0;
            continue;
        }
        int I[3];
        mg_coords<N>(L.n, id, I);
        double v[1 << N];
        el_cells_around<N>(L, I, v);
        double w[2 * N];
        int q[2 * N];
        bool edge[2 * N], rd[2 * N];      // the edge exists; its far node is free (its value is read)
#pragma unroll
        for (int d = 0; d < N; ++d)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int e = 2 * d + s;
                edge[e] = s ? I[d] < L.n[d] - 1 : I[d] > 0;
                q[e] = edge[e] ? (s ? id + cs[d] : id - cs[d]) : id;
                rd[e] = edge[e] && !L.fixed(q[e], 0);
                w[e] = (el_edge_sum<N>(v, d, s) * half) * L.ih2[d];
            }
        const double cm = el_cm<N>(L, id, I);
        for (int k = 0; k < ncols; ++k) {
            const double* __restrict__ xk = x + k * nn;
            const double xi = xk[id];
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < 2 * N; ++e) {
                const double xn = rd[e] ? xk[q[e]] : 0.0;
                if (edge[e]) acc = acc + w[e] * (xi - xn);
            }
            y[k * nn + id] = acc + cm * xi;
        }
    }
}

// ---- mode k into a field: x·scale rounded once to the storage type, exact zeros on the fixed nodes; the ghosts stay
template <int N>
__global__ void __launch_bounds__(MG_THREADS) elm_store_kernel(ElLevel L, MgField F, const double* __restrict__ x, double scale, void* __restrict__ u) {
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        st_val(u, mg_padded(F, I), F.f32, L.fixed(id, 0) ? 0.0 : x[id] * scale);
    }
}

// ---- g_I = e_I − (λ·ρ̄_I)·(u_I·u_I), u = the stored mode (x·scale rounded to the storage type).  e_I is el_energy_kernel's, the same
// operations in the same order on values read from x instead of a field; ρ̄_I = (Σ ρ_C over the existing cells, ascending from +0)/cells.
// c does not move with the shape: it gives no term
template <int N>
__global__ void __launch_bounds__(MG_THREADS) elm_sens_kernel(ElLevel L, MgField F, const double* __restrict__ x, double scale, double lam,
                                                              const double* __restrict__ rho, void* __restrict__ g_out) {
    const int cs[3] = {1, L.n[0], L.n[0] * L.n[1]};
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double v[1 << N];
        el_cells_around<N>(L, I, v);
        const double ui = em_round(x[id] * scale, F.f32);
        double e = 0.0;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            double ncell = 1.0;
#pragma unroll
            for (int o = 0; o < N; ++o)
                if (o != d && I[o] > 0 && I[o] < L.n[o] - 1) ncell = ncell * 2.0;
            double s = 0.0, cnt = 0.0;
            if (I[d] > 0) {
                const double g = (em_round(x[id - cs[d]] * scale, F.f32) - ui) / L.h[d];
                s = s + (el_edge_sum<N>(v, d, 0) / ncell) * (g * g);
                cnt = cnt + 1.0;
            }
            if (I[d] < L.n[d] - 1) {
                const double g = (em_round(x[id + cs[d]] * scale, F.f32) - ui) / L.h[d];
                s = s + (el_edge_sum<N>(v, d, 1) / ncell) * (g * g);
                cnt = cnt + 1.0;
            }
            e = e + s / cnt;
        }
        double rs = 0.0, nc = 0.0;
#pragma unroll
        for (int m = 0; m < (1 << N); ++m) {
            bool in;
            const double r = em_cell(L, rho, I, m, N, in);
            if (in) {
                rs = rs + r;
                nc = nc + 1.0;
            }
        }
        st_val(g_out, mg_padded(F, I), F.f32, e - (lam * (rs / nc)) * (ui * ui));
    }
}

}  // namespace lsm

struct LsmEllipticModes { LsmElliptic* e; ModesObject* o; };

int lsm_elliptic_modes_create(LsmElliptic* s, const void* phi, double level, double rho_in, double rho_out, const double* rho_cells, int m, LsmEllipticModes** out) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    EllipticObject& eo = *s->o;
    if (!out) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_create: null argument");
    if (!phi && !rho_cells) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_create: give phi or the cell densities");
    if (m < 1 || m > EM_MAXM) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_create: m must be between 1 and 8");
    if (3LL * m > eo.nfree) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_create: 3·m exceeds the number of free nodes");
    if (!rho_cells && (!(rho_in > 0) || !std::isfinite(rho_in) || !(rho_out > 0) || !std::isfinite(rho_out)))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_create: rho_in and rho_out must be finite and positive");
    if (!rho_cells && !std::isfinite(level)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_create: level must be finite");
    (void)hipSetDevice(h->device);
    std::unique_ptr<ModesObject> guard(new ModesObject());
    const int r = em_create(h, eo, *guard, "lsm_elliptic_modes_create", phi, level, rho_in, rho_out, rho_cells, m);
    if (r != LSM_OK) return r;
    *out = new LsmEllipticModes{s, guard.release()};
    return LSM_OK;
}

int lsm_elliptic_modes_mass(LsmEllipticModes* md, double* node_mass) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    if (!node_mass) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_mass: null argument");
    LSM_HIP(h, hipMemcpyAsync(node_mass, md->o->Mn, (size_t)md->e->o->lev[0].nn * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return LSM_OK;
}

static void elm_apply(const EllipticObject& eo, int ncols, const double* x, double* y, hipStream_t st) {
    const ElLevel& L = eo.lev[0];
    MG_LAUNCH(eo.N, elm_apply_kernel, mg_blocks(L.nn), MG_THREADS, st, L, ncols, x, y);
}

int lsm_elliptic_modes_apply(LsmEllipticModes* md, int ncols, const double* x, double* y) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    if (!x || !y || x == y) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_apply: x and y must be two arrays");
    if (ncols < 1 || ncols > EM_MAXM) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_apply: ncols must be between 1 and 8");
    elm_apply(*md->e->o, ncols, x, y, h->stream);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

int lsm_elliptic_modes_solve(LsmEllipticModes* md, const double* x0, double rtol, int max_iters, double* lambda, double* relres, int* iters, int64_t stats[4]) {
    if (!md) return LSM_ERR_INVALID;
    EllipticObject& eo = *md->e->o;
    return em_solve(md->e->h, eo, *md->o, "lsm_elliptic_modes_solve", [&](int na, const double* x, double* y, hipStream_t st) { elm_apply(eo, na, x, y, st); }, x0, rtol,
                    max_iters, lambda, relres, iters, stats);
}

int lsm_elliptic_modes_vectors(LsmEllipticModes* md, double* x_out) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    if (!x_out || !md->o->solved) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_vectors: null argument, or no solve has run");
    LSM_HIP(h, hipMemcpyAsync(x_out, md->o->B.base, (size_t)md->o->m * (size_t)md->o->nt * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return LSM_OK;
}

int lsm_elliptic_modes_store(LsmEllipticModes* md, int k, void* u) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    EllipticObject& eo = *md->e->o;
    ModesObject& o = *md->o;
    if (!o.solved || k < 0 || k >= o.m) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_store: no such mode, or no solve has run");
    if (!u) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_store: null field");
    const ElLevel& L = eo.lev[0];
    MG_LAUNCH(eo.N, elm_store_kernel, mg_blocks(L.nn), MG_THREADS, h->stream, L, eo.F, (const double*)(o.B.base + (size_t)k * o.nt), em_scale(L, eo.N), u);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

int lsm_elliptic_modes_sensitivity(LsmEllipticModes* md, int k, void* g_out) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    EllipticObject& eo = *md->e->o;
    ModesObject& o = *md->o;
    if (!o.solved || k < 0 || k >= o.m || !g_out) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elliptic_modes_sensitivity: no such mode, no solve has run, or a null field");
    const ElLevel& L = eo.lev[0];
    MG_LAUNCH(eo.N, elm_sens_kernel, mg_blocks(L.nn), MG_THREADS, h->stream, L, eo.F, (const double*)(o.B.base + (size_t)k * o.nt), em_scale(L, eo.N), o.lam[k],
              (const double*)o.rho, g_out);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

void lsm_elliptic_modes_destroy(LsmEllipticModes* md) {
    if (!md) return;
    delete md->o;
    delete md;
}
