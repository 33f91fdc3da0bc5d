// lsm_elastic.hip — elasticity_solve: −∇·σ(u) = f, σ = E(x)·C₀(ν):ε(u), on the box of a dense 2-D / 3-D grid with an ersatz material
// outside the level set: Q1 elements, the N displacement components at the nodes, traction-free faces, a caller-given set of fixed
// components; solved on the device by conjugate gradients preconditioned with one geometric multigrid V-cycle (or with the
// diagonal).  DESIGN.md §7.18; include/lsm.h ("elasticity_solve") states the discretisation, tests/_elastic_ref.py restates it.
// Built with -ffp-contract=off: the cell array, A x and the energy density round as numpy does.
//
// Storage.  Solver vectors are fp64, component-major: x[i·nn + id], id = i0 + n0·(i1 + n1·i2).  The cell moduli of a level have n−1
// entries per axis (lsm_elliptic.hip's cell array: el_cell.h is shared).  The operator is never stored: a node multiplies the unit
// element matrix K0 of its level — (2^N·N)² doubles in a small device buffer, read at compile-time offsets from a kernel argument,
// so through scalar loads — with the 3^N neighbours' components, cell by cell, and scales by the cell's modulus.  The diagonal is
// stored.  The fixed components hold zero in every vector the operator is applied to (search directions, smoother iterates), so
// the eliminated operator needs no mask on the neighbours; the rows of fixed components are set to zero.
//
// The PCG iteration and the V-cycle are mg_pcg.h's, with N components per node and ω = 0.6: D⁻¹A of Q1 elasticity has eigenvalues
// above 2/0.8 in 3-D, where the scalar solve's ω = 0.8 is no convergent smoother.  A level with stretched cells
// takes ω = 1.9/λ instead, λ its symbol bound on λmax(D⁻¹A), where that is smaller: with 0.6 there the V-cycle is indefinite.
// What is this file's own:
//   dir p = z + β p (a pass of its own, in place);  K1  q = A p,  σ = p·q   → α = ρ/σ
//
// The apply (K1, the residual, the smoother) is one thread per node with all N rows: the 3^N·N neighbour values are loaded once
// into registers (zero where there is no node), then 2^N cells × N rows × 2^N·N columns of multiply and add in the stated order.
#include <memory>

#include "el_cell.h"
#include "el_k0.h"
#include "lobpcg.h"
#include "mg_pcg.h"

namespace lsm {

static const double ES_OMEGA = 0.6;
static const double ES_SAFE = 1.9;      // ω·λmax(D⁻¹A) stays below 2 with this margin where ES_OMEGA would exceed it
enum { ES_BAD_PHI = 0, ES_BAD_E = 1, ES_NFIX = 2 /* 2, 3, 4: per component */, ES_NSTAT = 8 };

struct EsVec : MgVec { double* p; };     // the search direction, updated in place

struct EsLevel {
    int n[3];
    int nn;
    double h[3];
    const double* E;              // cell moduli, n−1 per axis
    const unsigned char* mask;    // one byte per node: bit i = component i is fixed
    const double* D;              // the diagonal, component-major
    const double* K;              // the level's K0, (2^N·N)² row-major
    double om;                    // the level's damping: min(ES_OMEGA, ES_SAFE/λ), λ the level's symbol bound (es_symbol_lambda)

    using Vec = EsVec;
    static constexpr int comps(int N) { return N; }
    __device__ __forceinline__ bool fixed(int id, int i) const { return (mask[id] >> i) & 1; }
    __device__ __forceinline__ double omega() const { return om; }
    static void launch_resid(int N, unsigned nb, hipStream_t s, const EsLevel& L, const double* r, const double* x, double* res, const MgState* st);
    static void launch_resid_many(int N, unsigned nb, unsigned cols, hipStream_t s, const EsLevel& L, const double* r, const double* x, double* res,
                                  const MgState* st);
    // the eliminated operator's N rows at a node; x holds zero on the fixed components, so there is nothing to mask
    template <int N, bool MASK>
    __device__ __forceinline__ void apply(int id, const int I[3], const double* x, int stride, double out[N]) const;
};

struct EsU { void* p[3]; };
// the fields of the columns of a batched solve (mg_pcg.h: the column is blockIdx.z) and their weights
struct EsUMany { void* p[MG_MAXCOLS][3]; };
struct EsW { double w[MG_MAXCOLS]; };
static_assert(MG_MAXCOLS == LSM_ELASTIC_MAXCOLS, "the batch of mg_pcg.h carries the columns that include/lsm.h promises");
template <class UT>
constexpr bool es_many = std::is_same<UT, EsUMany>::value;
__device__ __forceinline__ void* es_u(const EsU& U, int i) { return U.p[i]; }
__device__ __forceinline__ void* es_u(const EsUMany& U, int i) { return U.p[blockIdx.z][i]; }

// cell m of the 2^N around node I (bit d of m set: cell index I_d along d, clear: I_d − 1): its modulus, or zero where there is none
template <int N>
__device__ __forceinline__ double es_cell(const EsLevel& L, const int I[3], int m, bool& in) {
    int C[3] = {0, 0, 0};
    in = true;
#pragma unroll
    for (int d = 0; d < N; ++d) {
        C[d] = I[d] - 1 + ((m >> d) & 1);
        in = in && C[d] >= 0 && C[d] < L.n[d] - 1;
    }
    return in ? L.E[mg_cell_index<N>(L.n, C)] : 0.0;
}

// (A x)_{I,·} in the stated order: the cells ascending; per cell and row the columns from +0, corner b ascending, component j
// fastest; then the cell's modulus; the cell terms from +0.  xat(q, o0, o1, o2, j): component j at the node q = I + o, which exists.
// A cell that does not exist has E = 0 and its missing nodes the value 0: it adds ±0 to a sum that began at +0.
template <int N, class X>
__device__ __forceinline__ void es_apply(const EsLevel& L, int id, const int I[3], X xat, double out[N]) {
    constexpr int NC = 1 << N, NB = N == 2 ? 9 : 27, R = NC * N;
    const int s1 = L.n[0], s2 = N > 2 ? L.n[0] * L.n[1] : 0;
    bool lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        lo[d] = d < N && I[d] > 0;
        hi[d] = d < N && I[d] < L.n[d] - 1;
    }
    double v[NB][N];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int o0 = k % 3 - 1, o1 = (k / 3) % 3 - 1, o2 = N > 2 ? k / 9 - 1 : 0;
        const bool ex = (o0 >= 0 || lo[0]) && (o0 <= 0 || hi[0]) && (o1 >= 0 || lo[1]) && (o1 <= 0 || hi[1]) && (o2 >= 0 || lo[2]) && (o2 <= 0 || hi[2]);
        const int q = id + o0 + o1 * s1 + o2 * s2;
#pragma unroll
        for (int j = 0; j < N; ++j) v[k][j] = 0.0;
        if (ex) {
#pragma unroll
            for (int j = 0; j < N; ++j) v[k][j] = xat(q, o0, o1, o2, j);
        }
    }
    const double* __restrict__ K = L.K;
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = 0.0;
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        bool in;
        const double E = es_cell<N>(L, I, m, in);
        const int a = (~m) & (NC - 1);
        double inner[N];
#pragma unroll
        for (int i = 0; i < N; ++i) inner[i] = 0.0;
#pragma unroll
        for (int b = 0; b < NC; ++b) {
            const int o0 = (m & 1) + (b & 1) - 1, o1 = ((m >> 1) & 1) + ((b >> 1) & 1) - 1, o2 = N > 2 ? ((m >> 2) & 1) + ((b >> 2) & 1) - 1 : 0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double val = v[(o0 + 1) + 3 * (o1 + 1) + (N > 2 ? 9 * (o2 + 1) : 0)][j];
#pragma unroll
                for (int i = 0; i < N; ++i) inner[i] = inner[i] + K[(a * N + i) * R + b * N + j] * val;
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) out[i] = out[i] + E * inner[i];
    }
}

template <int N, bool MASK>
__device__ __forceinline__ void EsLevel::apply(int id, const int I[3], const double* x, int stride, double out[N]) const {
    es_apply<N>(*this, id, I, [&](int q, int, int, int, int j) { return x[j * stride + q]; }, out);
}

// ---- setup of level 0: the cell moduli from ϕ (or the caller's, checked), the fixed bits counted per component
template <int N>
__global__ void __launch_bounds__(MG_THREADS) es_setup_kernel(EsLevel L, MgField F, const void* __restrict__ phi, double level, double e_in, double e_out,
                                                              double hmin, const double* __restrict__ e_given, double* __restrict__ E, unsigned long long* st) {
    unsigned cnt[5] = {0, 0, 0, 0, 0};
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        if (phi && !mg_finite(ld_val(phi, mg_padded(F, I), F.f32))) ++cnt[ES_BAD_PHI];
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (L.fixed(id, i)) ++cnt[ES_NFIX + i];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && I[d] < L.n[d] - 1;
        if (!corner) continue;
        const int ci = I[0] + (L.n[0] - 1) * (I[1] + (N > 2 ? (L.n[1] - 1) * I[2] : 0));
        double ev;
        if (e_given) {
            ev = e_given[ci];
            if (!(ev > 0.0) || !mg_finite(ev)) ++cnt[ES_BAD_E];
        } else {
            ev = el_cell_from_phi<N>(phi, mg_padded(F, I), F.s1, F.s2, F.f32, level, e_in, e_out, hmin);
            if (!(ev > 0.0)) ++cnt[ES_BAD_E];
        }
        E[ci] = ev;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned v = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&st[k], (unsigned long long)v);
    }
}

// ---- a coarse level from the fine one: cells averaged, the fixed bits of fine node 2J.  co: the axes that coarsen
template <int N>
__global__ void __launch_bounds__(MG_THREADS) es_coarsen_kernel(EsLevel Lf, EsLevel Lc, int co0, int co1, int co2, double* __restrict__ Ec,
                                                                unsigned char* __restrict__ fixc) {
    const int co[3] = {co0, co1, co2};
    const double scale = mg_coarsen_scale(co0 + co1 + co2);
    MG_LOOP(id, Lc.nn) {
        int J[3];
        mg_coords<N>(Lc.n, id, J);
        const int fid = (co[0] ? 2 * J[0] : J[0]) + Lf.n[0] * ((co[1] ? 2 * J[1] : J[1]) + (N > 2 ? Lf.n[1] * (co[2] ? 2 * J[2] : J[2]) : 0));
        fixc[id] = Lf.mask[fid];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && J[d] < Lc.n[d] - 1;
        if (!corner) continue;
        Ec[mg_cell_index<N>(Lc.n, J)] = mg_cell_average<N>(Lf.E, Lf.n, J, co, scale);
    }
}

// ---- the diagonal of a level: D_{I,i} = Σ_C E_C·K0[(a,i),(a,i)]
template <int N>
__global__ void __launch_bounds__(MG_THREADS) es_diag_kernel(EsLevel L, double* __restrict__ D) {
    constexpr int NC = 1 << N, R = NC * N;
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double acc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = 0.0;
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            bool in;
            const double E = es_cell<N>(L, I, m, in);
            const int a = (~m) & (NC - 1);
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] = acc[i] + E * L.K[(a * N + i) * R + a * N + i];
        }
#pragma unroll
        for (int i = 0; i < N; ++i) D[i * L.nn + id] = acc[i];
    }
}

// ---- y = A x on all components, no elimination (lsm_elastic_apply)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) es_apply_kernel(EsLevel L, const double* __restrict__ x, double* __restrict__ y) {
    const int nn = L.nn;
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double out[N];
        es_apply<N>(L, id, I, [&](int q, int, int, int, int j) { return x[j * nn + q]; }, out);
#pragma unroll
        for (int i = 0; i < N; ++i) y[i * nn + id] = out[i];
    }
}

// ---- the energy density e_I = (Σ_C E_C·q_C)/(existing cells around I), q_C = Σ_r u_r·(Σ_s K0[r,s]·u_s), into a field of the handle
template <int N>
__global__ void __launch_bounds__(MG_THREADS) es_energy_kernel(EsLevel L, MgField F, EsU U, void* __restrict__ e_out) {
    constexpr int NC = 1 << N, R = NC * N;
    const double* __restrict__ K = L.K;
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
        double acc = 0.0, cnt = 0.0;
#pragma unroll 1
        for (int m = 0; m < NC; ++m) {
            bool in;
            const double E = es_cell<N>(L, I, m, in);
            if (!in) continue;
            const long long c0 = at + ((m & 1) - 1) + (((m >> 1) & 1) - 1) * F.s1 + (N > 2 ? (((m >> 2) & 1) - 1) * F.s2 : 0);     // the cell's lowest corner
            double uc[R];
#pragma unroll
            for (int b = 0; b < NC; ++b) {
                const long long o = (b & 1) + ((b >> 1) & 1) * F.s1 + (N > 2 ? ((b >> 2) & 1) * F.s2 : 0);
#pragma unroll
                for (int j = 0; j < N; ++j) uc[b * N + j] = ld_val(U.p[j], c0 + o, F.f32);
            }
            double q = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double t = 0.0;
#pragma unroll
                for (int s = 0; s < R; ++s) t = t + K[r * R + s] * uc[s];
                q = q + uc[r] * t;
            }
            acc = acc + E * q;
            cnt = cnt + 1.0;
        }
        st_val(e_out, at, F.f32, acc / cnt);
    }
}

// ---- the weighted energy density of K columns in one pass: e_I = Σ_k w_k·e_{k,I} (k ascending, from +0), e_{k,I} es_energy_kernel's value of
// column k in fp64.  A node loops over its cells and, inside, over the columns: the cell's modulus is read once for all of them.  The K
// accumulators of a lane live in LDS (a column each, indexed by the loop's k): as a register array they would be indexed dynamically
template <int N>
__global__ void __launch_bounds__(MG_THREADS) es_energy_many_kernel(EsLevel L, MgField F, EsUMany U, int ncol, EsW W, void* __restrict__ e_out) {
    constexpr int NC = 1 << N, R = NC * N;
    __shared__ double accs[MG_MAXCOLS][MG_THREADS];
    const double* __restrict__ K = L.K;
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
#pragma unroll 1
        for (int k = 0; k < ncol; ++k) accs[k][threadIdx.x] = 0.0;
        double cnt = 0.0;
#pragma unroll 1
        for (int m = 0; m < NC; ++m) {
            bool in;
            const double E = es_cell<N>(L, I, m, in);
            if (!in) continue;
            const long long c0 = at + ((m & 1) - 1) + (((m >> 1) & 1) - 1) * F.s1 + (N > 2 ? (((m >> 2) & 1) - 1) * F.s2 : 0);     // the cell's lowest corner
#pragma unroll 1
            for (int k = 0; k < ncol; ++k) {
                double uc[R];
#pragma unroll
                for (int b = 0; b < NC; ++b) {
                    const long long o = (b & 1) + ((b >> 1) & 1) * F.s1 + (N > 2 ? ((b >> 2) & 1) * F.s2 : 0);
#pragma unroll
                    for (int j = 0; j < N; ++j) uc[b * N + j] = ld_val(U.p[k][j], c0 + o, F.f32);
                }
                double q = 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    double t = 0.0;
#pragma unroll
                    for (int s = 0; s < R; ++s) t = t + K[r * R + s] * uc[s];
                    q = q + uc[r] * t;
                }
                accs[k][threadIdx.x] = accs[k][threadIdx.x] + E * q;
            }
            cnt = cnt + 1.0;
        }
        double e = 0.0;
#pragma unroll 1
        for (int k = 0; k < ncol; ++k) e = e + W.w[k] * (accs[k][threadIdx.x] / cnt);
        st_val(e_out, at, F.f32, e);
    }
}

// ---- the mutual energy density m_I = (Σ_C E_C·q_C)/(existing cells around I), q_C = Σ_r u_r·(Σ_s K0[r,s]·v_s): es_energy_kernel's sums with v
// in the inner one, so that v = u gives its bits
template <int N>
__global__ void __launch_bounds__(MG_THREADS) es_energy_mutual_kernel(EsLevel L, MgField F, EsU U, EsU V, void* __restrict__ e_out) {
    constexpr int NC = 1 << N, R = NC * N;
    const double* __restrict__ K = L.K;
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
        double acc = 0.0, cnt = 0.0;
#pragma unroll 1
        for (int m = 0; m < NC; ++m) {
            bool in;
            const double E = es_cell<N>(L, I, m, in);
            if (!in) continue;
            const long long c0 = at + ((m & 1) - 1) + (((m >> 1) & 1) - 1) * F.s1 + (N > 2 ? (((m >> 2) & 1) - 1) * F.s2 : 0);     // the cell's lowest corner
            double uc[R], vc[R];
#pragma unroll
            for (int b = 0; b < NC; ++b) {
                const long long o = (b & 1) + ((b >> 1) & 1) * F.s1 + (N > 2 ? ((b >> 2) & 1) * F.s2 : 0);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    uc[b * N + j] = ld_val(U.p[j], c0 + o, F.f32);
                    vc[b * N + j] = ld_val(V.p[j], c0 + o, F.f32);
                }
            }
            double q = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double t = 0.0;
#pragma unroll
                for (int s = 0; s < R; ++s) t = t + K[r * R + s] * vc[s];
                q = q + uc[r] * t;
            }
            acc = acc + E * q;
            cnt = cnt + 1.0;
        }
        st_val(e_out, at, F.f32, acc / cnt);
    }
}

// ---- Πh·Σ b·u is finished on the host: this reduces Σ (m·f)·u over the components
template <int N>
__global__ void __launch_bounds__(MG_THREADS) es_compliance_kernel(EsLevel L, MgField F, const double* __restrict__ f, EsU U, double* partial, MgState* st) {
    double red[1] = {0.0};
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const double m = mg_mass<N>(L.n, I);
        const long long at = mg_padded(F, I);
#pragma unroll
        for (int i = 0; i < N; ++i) red[0] += (m * f[i * L.nn + id]) * ld_val(U.p[i], at, F.f32);
    }
    if (!block_reduce_ordered<1, MG_THREADS>(red, partial, &st->ticket[3]) || threadIdx.x != 0) return;
    st->out = red[0];
}

// ---- PCG
// x₀ = u (the guess and the prescribed values) as fp64, p = 0
template <int N, class UT = EsU>
__global__ void __launch_bounds__(MG_THREADS) es_load_kernel(EsLevel L, MgField F, EsVec V, UT U) {
    const int nn = L.nn;
    if constexpr (es_many<UT>) {
        const size_t at = (size_t)blockIdx.z * N * nn;
        V.x += at; V.p += at;
    }
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            V.x[i * nn + id] = ld_val(es_u(U, i), at, F.f32);
            V.p[i * nn + id] = 0.0;
        }
    }
}
// b = m·f, r₀ = b − A x₀ on the free components, 0 on the fixed ones; ‖b_free‖², ‖r₀‖²; jac: z = r/D and ρ = r·z as well
template <int N, int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) es_init_kernel(EsLevel L, EsVec V, const double* __restrict__ x, const double* __restrict__ f,
                                                             double* __restrict__ rv, double* __restrict__ zv, int jac) {
    double red[4] = {0.0, 0.0, 0.0, 0.0};     // ‖b_free‖², ‖r₀‖², r·z, non-finite entries (a count below 2^53: exact)
    const int nn = L.nn;
    if constexpr (MANY) {
        const size_t c = blockIdx.z, at = c * N * nn;
        x += at; f += at; rv += at; zv += at;
        V.partial += c * (4 * MG_MAXB);
        V.st += c;
    }
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const double m = mg_mass<N>(L.n, I);
        double out[N];
        es_apply<N>(L, id, I, [&](int q, int, int, int, int j) { return x[j * nn + q]; }, out);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double ui = x[i * nn + id], fi = f[i * nn + id];
            if (!mg_finite(ui) || !mg_finite(fi)) red[3] += 1.0;
            double r = 0.0, z = 0.0;
            if (!L.fixed(id, i)) {
                const double b = m * fi;
                r = b - out[i];
                red[0] += b * b;
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

// the search direction over the nt = N·nn unknowns, in place: p = z + β p (z and p are zero on the fixed components, so p stays zero there)
template <int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) es_dir_kernel(int nt, EsVec V) {
    if constexpr (MANY) {
        const size_t at = (size_t)blockIdx.z * nt;
        V.z += at; V.p += at;
        V.st += blockIdx.z;
    }
    if (V.st->status != MG_RUN) return;
    const double beta = V.st->beta;
    const double* __restrict__ z = V.z;
    double* __restrict__ p = V.p;
    MG_LOOP(k, nt) p[k] = z[k] + beta * p[k];
}
// K1: q = A p, σ = p·q, α = ρ/σ.  The direction has a pass of its own, in place: one vector less than lsm_elliptic.hip's double-buffered
// p, and the apply loads 3^N·N values, not twice as many.  The vectors are __restrict__ parameters, not fields of V: read through
// the struct, this kernel and es_init_kernel compiled to 3.2 KB of scratch per lane in 3-D.
template <int N, int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) es_k1_kernel(EsLevel L, const double* __restrict__ p, double* __restrict__ qv, double* partial, MgState* st) {
    if constexpr (MANY) {
        const size_t c = blockIdx.z, at = c * N * L.nn;
        p += at; qv += at;
        partial += c * (4 * MG_MAXB);
        st += c;
    }
    if (st->status != MG_RUN) return;
    const int nn = L.nn;
    double red[1] = {0.0};
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double out[N];
        es_apply<N>(L, id, I, [&](int q, int, int, int, int j) { return p[j * nn + q]; }, out);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double q = 0.0;
            if (!L.fixed(id, i)) {
                q = out[i];
                red[0] += p[i * nn + id] * q;
            }
            qv[i * nn + id] = q;
        }
    }
    if (!block_reduce_ordered<1, MG_THREADS>(red, partial, &st->ticket[1]) || threadIdx.x != 0) return;
    mg_k1_tail(*st, red[0]);
}

// ---- x → u on the free components (rounded to the storage type); the fixed components and the ghosts are left as they are
template <int N, class UT = EsU>
__global__ void __launch_bounds__(MG_THREADS) es_store_kernel(EsLevel L, MgField F, const double* __restrict__ x, UT U) {
    if constexpr (es_many<UT>) x += (size_t)blockIdx.z * N * L.nn;
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (!L.fixed(id, i)) st_val(es_u(U, i), at, F.f32, x[i * L.nn + id]);
    }
}

// the V-cycle's fine residual in 2-D, zero on the fixed components.  mg_resid_kernel<2, EsLevel> is the same loop with the operator
// called through EsLevel::apply, and compiled to 106 SGPRs where this form takes 98: one wave per SIMD less.
template <int MANY = 0>
__global__ void __launch_bounds__(MG_THREADS) es_resid2_kernel(EsLevel L, const double* __restrict__ r, const double* __restrict__ x, double* __restrict__ res,
                                                               const MgState* st) {
    if constexpr (MANY) {
        const size_t at = (size_t)blockIdx.z * 2 * L.nn;
        r += at; x += at; res += at;
        st += blockIdx.z;
    }
    if (st->status != MG_RUN) return;
    const int nn = L.nn;
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<2>(L.n, id, I);
        double out[2];
        es_apply<2>(L, id, I, [&](int q, int, int, int, int j) { return x[j * nn + q]; }, out);
#pragma unroll
        for (int i = 0; i < 2; ++i) res[i * nn + id] = L.fixed(id, i) ? 0.0 : r[i * nn + id] - out[i];
    }
}

// ---- host side
void EsLevel::launch_resid(int N, unsigned nb, hipStream_t s, const EsLevel& L, const double* r, const double* x, double* res, const MgState* st) {
    if (N == 2) hipLaunchKernelGGL(es_resid2_kernel<>, dim3(nb), dim3(MG_THREADS), 0, s, L, r, x, res, st);
    else hipLaunchKernelGGL((mg_resid_kernel<3, EsLevel>), dim3(nb), dim3(MG_THREADS), 0, s, L, r, x, res, st);
}
void EsLevel::launch_resid_many(int N, unsigned nb, unsigned cols, hipStream_t s, const EsLevel& L, const double* r, const double* x, double* res,
                                const MgState* st) {
    if (N == 2) hipLaunchKernelGGL(es_resid2_kernel<1>, dim3(nb, 1, cols), dim3(MG_THREADS), 0, s, L, r, x, res, st);
    else hipLaunchKernelGGL((mg_resid_kernel<3, EsLevel, 1>), dim3(nb, 1, cols), dim3(MG_THREADS), 0, s, L, r, x, res, st);
}
struct ElasticObject : MgSolver<EsLevel> {
    std::vector<std::vector<double>> k0; // the levels' K0 as computed (what the device holds)
    double lam = 0.0, mu = 0.0;          // the material at E = 1 (plane-dependent), for the stress recovery
    int plane = 0;
    // the batched solve's workspace: the vectors, states and partials of `cols` columns, with the levels (the operator's data) shared.
    // Made by the first lsm_elastic_solve_many, grown when a later one asks for more columns; the single solve's workspace is not touched
    std::unique_ptr<MgSolver<EsLevel>> many;
};

// the unit element matrix of a box cell with sides h, scaled by 1/∏h (include/lsm.h states the formula): a product over the axes
// of the 1-D factors mass h/3 | h/6, stiffness ±1/h, mixed ±½ (the sign of the differentiated corner)
void es_k0(int N, const double h[3], double lam, double mu, std::vector<double>& K) {
    const int NC = 1 << N, R = NC * N;
    std::vector<double> G((size_t)NC * NC * N * N);
    auto g_at = [&](int a, int b, int i, int j) -> double& { return G[(((size_t)a * NC + b) * N + i) * N + j]; };
    double vol = 1.0;
    for (int d = 0; d < N; ++d) vol = vol * h[d];
    for (int a = 0; a < NC; ++a)
        for (int b = 0; b < NC; ++b)
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) {
                    double g = 1.0;
                    for (int d = 0; d < N; ++d) {
                        const int ad = (a >> d) & 1, bd = (b >> d) & 1;
                        if (i == j && d == i) g = g * ((ad == bd ? 1.0 : -1.0) / h[d]);
                        else if (i != j && d == i) g = g * (ad ? 0.5 : -0.5);
                        else if (i != j && d == j) g = g * (bd ? 0.5 : -0.5);
                        else g = g * (ad == bd ? h[d] / 3.0 : h[d] / 6.0);
                    }
                    g_at(a, b, i, j) = g;
                }
    K.assign((size_t)R * R, 0.0);
    for (int a = 0; a < NC; ++a)
        for (int b = 0; b < NC; ++b) {
            double tr = 0.0;
            for (int k = 0; k < N; ++k) tr = tr + g_at(a, b, k, k);
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) {
                    double v = lam * g_at(a, b, i, j) + mu * g_at(a, b, j, i);
                    if (i == j) v = v + mu * tr;
                    K[(size_t)(a * N + i) * R + b * N + j] = v / vol;
                }
        }
}

// λmax(D⁻¹A) of the level's operator on a uniform infinite grid, from K0 alone: the largest eigenvalue over the 2^N corner
// frequencies θ ∈ {0, π}^N of the N×N symbol D^−½·Â(θ)·D^−½, Â_ij(θ) = Σ_a Σ_b ±K0[(a,i),(b,j)] (minus where a and b differ on an odd
// number of the axes with θ_d = π), D_i = Σ_a K0[(a,i),(a,i)].  Stretched cells — an axis that stopped coarsening while the others go
// on — push it past 2/ES_OMEGA, where damped Jacobi amplifies and the V-cycle is no longer positive definite.
double es_symbol_lambda(int N, const std::vector<double>& K) {
    const int NC = 1 << N, R = NC * N;
    double D[3] = {0, 0, 0}, best = 0.0;
    for (int i = 0; i < N; ++i)
        for (int a = 0; a < NC; ++a) D[i] += K[(size_t)(a * N + i) * R + a * N + i];
    for (int th = 0; th < NC; ++th) {
        double A[3][3] = {{0}};
        for (int a = 0; a < NC; ++a)
            for (int b = 0; b < NC; ++b) {
                const double sg = (__builtin_popcount((a ^ b) & th) & 1) ? -1.0 : 1.0;
                for (int i = 0; i < N; ++i)
                    for (int j = 0; j < N; ++j) A[i][j] += sg * K[(size_t)(a * N + i) * R + b * N + j] / std::sqrt(D[i] * D[j]);
            }
        double x[3] = {1.0, 0.9, 0.8}, lam = 0.0;     // power iteration: the symbol is symmetric and not negative
        for (int it = 0; it < 500; ++it) {
            double y[3] = {0, 0, 0}, nrm = 0.0;
            for (int i = 0; i < N; ++i) {
                for (int j = 0; j < N; ++j) y[i] += A[i][j] * x[j];
                nrm += y[i] * y[i];
            }
            nrm = std::sqrt(nrm);
            if (!(nrm > 0.0)) break;
            lam = nrm;
            for (int i = 0; i < N; ++i) x[i] = y[i] / nrm;
        }
        best = std::max(best, lam);
    }
    return best;
}

}  // namespace lsm

using namespace lsm;

struct LsmElastic { LsmHandle* h; ElasticObject* o; };

static int es_create(LsmHandle* h, ElasticObject& o, const void* phi, double level, double e_in, double e_out, const double* e_cells, double lam, double mu,
                     const unsigned char* fixed, int64_t stats[4]) {
    const int N = h->grid.ndim;
    o.N = N;
    o.F = MgField{h->lay.stride[1], N > 2 ? h->lay.stride[2] : 0, h->lay.origin, h->dtype == LSM_DTYPE_F32 ? 1 : 0};
    std::vector<EsLevel> lev;
    EsLevel L;
    memset(&L, 0, sizeof(L));
    double hmin;
    const long long nn = mg_shapes(h, L, 1LL << 28, lev, o.co, hmin);
    if (lev.empty()) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: the grid is too large (2^28 nodes at most)");
    const int nl = (int)lev.size();
    if (lev[nl - 1].nn > 128) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: the coarsest level has more than 128 nodes");
    const size_t RR = (size_t)((1 << N) * N) * (size_t)((1 << N) * N);
    // one allocation of doubles: per level K0, cells, D, xa, xb, [rhs]; level 0: x r q p as well
    size_t nd = 0, nb = 0;
    for (int l = 0; l < nl; ++l) {
        nd += RR + mg_ncells(N, lev[l]) + (size_t)N * (size_t)lev[l].nn * (size_t)(3 + (l ? 1 : 4));
        nb += (size_t)lev[l].nn;
    }
    LSM_HIP(h, o.buf.alloc(nd * sizeof(double)));
    LSM_HIP(h, o.fx.alloc(nb));
    hipStream_t s = h->stream;
    const int ra = mg_alloc_scalars(h, o, ES_NSTAT, s);
    if (ra != LSM_OK) return ra;
    double* b = o.buf;
    unsigned char* fb = o.fx;
    std::vector<double*> ecell(nl), dg(nl), kd(nl);
    std::vector<unsigned char*> fxl(nl, nullptr);
    o.rhs.assign(nl, nullptr); o.xa.assign(nl, nullptr); o.xb.assign(nl, nullptr);
    o.k0.resize(nl);
    for (int l = 0; l < nl; ++l) {
        const size_t m = (size_t)N * (size_t)lev[l].nn;
        kd[l] = b; b += RR;
        ecell[l] = b; b += mg_ncells(N, lev[l]);
        dg[l] = b; b += m;
        o.xa[l] = b; b += m;
        o.xb[l] = b; b += m;
        if (l) { o.rhs[l] = b; b += m; }
        else {
            o.V.x = b; b += m; o.V.r = b; b += m; o.V.q = b; b += m; o.V.p = b; b += m;
        }
        fxl[l] = fb; fb += lev[l].nn;
        lev[l].E = ecell[l]; lev[l].D = dg[l]; lev[l].K = kd[l]; lev[l].mask = fxl[l];
        es_k0(N, lev[l].h, lam, mu, o.k0[l]);       // o.k0 outlives the copy: it belongs to the object
        lev[l].om = std::min(ES_OMEGA, ES_SAFE / es_symbol_lambda(N, o.k0[l]));
        LSM_HIP(h, hipMemcpyAsync(kd[l], o.k0[l].data(), RR * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (fixed) LSM_HIP(h, hipMemcpyAsync(fxl[0], fixed, (size_t)nn, hipMemcpyDeviceToDevice, s));
    else LSM_HIP(h, hipMemsetAsync(fxl[0], 0, (size_t)nn, s));
    MG_LAUNCH(N, es_setup_kernel, dim3(mg_blocks(nn)), MG_THREADS, s, lev[0], o.F, e_cells ? (const void*)nullptr : phi, level, e_in, e_out, hmin, e_cells,
              ecell[0], o.cnt.p);
    LSM_HIP(h, hipGetLastError());
    unsigned long long c[ES_NSTAT] = {};
    LSM_HIP(h, hipMemcpyAsync(c, o.cnt.p, sizeof(c), hipMemcpyDeviceToHost, s));
    LSM_HIP(h, hipStreamSynchronize(s));
    o.nfixed = 0;
    int unfixed = -1;
    for (int i = N - 1; i >= 0; --i) {
        o.nfixed += (long long)c[ES_NFIX + i];
        if (!c[ES_NFIX + i]) unfixed = i;
    }
    o.nfree = (long long)N * nn - o.nfixed;
    // what the data is refused for: stats = {-(reason), offending entries (reason 4: the component), 0, 0}
    const int reason = c[ES_BAD_PHI] ? 1 : c[ES_BAD_E] ? 2 : unfixed >= 0 ? 4 : o.nfree == 0 ? 5 : 0;
    if (reason) {
        static const char* why[5] = {"lsm_elastic_create: phi must be finite", "lsm_elastic_create: the cell moduli must be finite and positive", "",
                                     "lsm_elastic_create: a displacement component has no fixed bit anywhere (its translation is in the null space)",
                                     "lsm_elastic_create: every component of every node is fixed"};
        if (stats) { stats[0] = -reason; stats[1] = (int64_t)(reason == 1 ? c[ES_BAD_PHI] : reason == 2 ? c[ES_BAD_E] : reason == 4 ? unfixed : 0); stats[2] = stats[3] = 0; }
        return lsm_fail(h, LSM_ERR_INVALID, why[reason - 1]);
    }
    for (int l = 1; l < nl; ++l)
        MG_LAUNCH(N, es_coarsen_kernel, dim3(mg_blocks(lev[l].nn)), MG_THREADS, s, lev[l - 1], lev[l], o.co[l - 1][0], o.co[l - 1][1], o.co[l - 1][2], ecell[l],
                  fxl[l]);
    for (int l = 0; l < nl; ++l) MG_LAUNCH(N, es_diag_kernel, dim3(mg_blocks(lev[l].nn)), MG_THREADS, s, lev[l], dg[l]);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(s));
    o.lev = lev;
    o.V.z = o.precond == LSM_PRECOND_JACOBI ? o.xa[0] : o.xb[0];
    if (stats) { stats[0] = nl; stats[1] = o.nfree; stats[2] = o.nfixed; stats[3] = 0; }
    return LSM_OK;
}

int lsm_elastic_create(LsmHandle* h, const void* phi, double level, double e_in, double e_out, const double* e_cells, double nu, int plane, const void* fixed,
                       int precond, LsmElastic** out, int64_t stats[4]) {
    if (!h || !out) return h ? lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: null argument") : LSM_ERR_INVALID;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (!phi && !e_cells) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: give phi or the cell moduli");
    const int N = h->grid.ndim;
    if (N == 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: a 1-dimensional grid is not supported (2-D and 3-D only)");
    if (h->comm) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: the handle has a communicator attached (single device only)");
    if (h->bc[N - 1][0].kind == LSM_BC_NONE || h->bc[N - 1][1].kind == LSM_BC_NONE)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: the handle is a slab of a multi-GPU grid (whole grids only)");
    for (int d = 0; d < N; ++d) {
        if (h->bc[d][0].kind == LSM_BC_PERIODIC || h->bc[d][1].kind == LSM_BC_PERIODIC)
            return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: a periodic dimension is not supported (the faces are traction-free)");
        if (h->nloc[d] < 3) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: at least 3 nodes per dimension");
    }
    if (!e_cells && (!(e_in > 0) || !std::isfinite(e_in) || !(e_out > 0) || !std::isfinite(e_out)))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: e_in and e_out must be finite and positive");
    if (!e_cells && !std::isfinite(level)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: level must be finite");
    if (!std::isfinite(nu) || !(nu > -1.0) || !(nu < 0.5)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: nu must be finite with -1 < nu < 0.5");
    if (plane != LSM_PLANE_STRESS && plane != LSM_PLANE_STRAIN) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: unknown plane (LSM_PLANE_STRESS or LSM_PLANE_STRAIN)");
    if (precond != LSM_PRECOND_MG && precond != LSM_PRECOND_JACOBI) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_create: unknown preconditioner");
    const double mu = 1.0 / (2.0 * (1.0 + nu));
    const double lam = (N == 2 && plane == LSM_PLANE_STRESS) ? nu / (1.0 - nu * nu) : nu / ((1.0 + nu) * (1.0 - 2.0 * nu));
    (void)hipSetDevice(h->device);
    ElasticObject* o = new ElasticObject();
    o->precond = precond;
    o->lam = lam; o->mu = mu; o->plane = plane;
    const int r = es_create(h, *o, phi, level, e_in, e_out, e_cells, lam, mu, (const unsigned char*)fixed, stats);
    if (r != LSM_OK) { delete o; return r; }
    *out = new LsmElastic{h, o};
    return LSM_OK;
}

int lsm_elastic_stiffness(LsmElastic* s, int level, double* k0_host) {
    if (!s) return LSM_ERR_INVALID;
    if (!k0_host || level < 0 || level >= (int)s->o->k0.size()) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stiffness: no such level, or a null array");
    memcpy(k0_host, s->o->k0[level].data(), s->o->k0[level].size() * sizeof(double));
    return LSM_OK;
}

int lsm_elastic_apply(LsmElastic* s, const double* x, double* y) {
    if (!s) return LSM_ERR_INVALID;
    if (!x || !y || x == y) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_apply: x and y must be two arrays");
    const EsLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, es_apply_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, x, y);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_cells(LsmElastic* s, double* e_out_cells) {
    if (!s) return LSM_ERR_INVALID;
    if (!e_out_cells) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_cells: null argument");
    const EsLevel& L = s->o->lev[0];
    const size_t m = mg_ncells(s->o->N, L);
    LSM_HIP(s->h, hipMemcpyAsync(e_out_cells, L.E, m * sizeof(double), hipMemcpyDeviceToDevice, s->h->stream));
    return LSM_OK;
}

// the N fields of u: all given, no two the same
static bool es_fields(int N, const void* u0, const void* u1, const void* u2, EsU& U) {
    U.p[0] = (void*)u0; U.p[1] = (void*)u1; U.p[2] = N > 2 ? (void*)u2 : nullptr;
    if (!u0 || !u1 || u0 == u1) return false;
    if (N > 2 && (!u2 || u2 == u0 || u2 == u1)) return false;
    return true;
}

int lsm_elastic_energy(LsmElastic* s, const void* u0, const void* u1, const void* u2, void* e_out) {
    if (!s) return LSM_ERR_INVALID;
    EsU U;
    if (!es_fields(s->o->N, u0, u1, u2, U) || !e_out || e_out == u0 || e_out == u1 || e_out == u2)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_energy: the components of u and e_out must be distinct fields");
    const EsLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, es_energy_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, s->o->F, U, e_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_compliance(LsmElastic* s, const double* f, const void* u0, const void* u1, const void* u2, double* out) {
    if (!s) return LSM_ERR_INVALID;
    EsU U;
    if (!f || !out || !es_fields(s->o->N, u0, u1, u2, U)) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_compliance: null argument");
    ElasticObject& o = *s->o;
    const EsLevel& L = o.lev[0];
    hipStream_t st = s->h->stream;
    MG_LAUNCH(o.N, es_compliance_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, o.F, f, U, o.partial.p, o.st.p);
    LSM_HIP(s->h, hipGetLastError());
    LSM_HIP(s->h, hipMemcpyAsync(o.h_st, o.st, sizeof(MgState), hipMemcpyDeviceToHost, st));
    LSM_HIP(s->h, hipStreamSynchronize(st));
    double vol = 1.0;
    for (int d = 0; d < o.N; ++d) vol *= L.h[d];
    *out = vol * o.h_st.p->out;
    return LSM_OK;
}

int lsm_elastic_solve(LsmElastic* s, const double* f, void* u0, void* u1, void* u2, double rtol, int max_iters, int* iters_out, double* relres_out, void* stream) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    ElasticObject& o = *s->o;
    EsU U;
    if (!f || !es_fields(o.N, u0, u1, u2, U)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_solve: f and the N distinct fields of u must be given");
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_solve: rtol must be positive and max_iters at least 1");
    const int N = o.N;
    const EsLevel& L = o.lev[0];
    const int jac = o.precond == LSM_PRECOND_JACOBI;
    (void)hipSetDevice(h->device);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const int r0 = mg_reset(h, o, rtol, max_iters, st);
    if (r0 != LSM_OK) return r0;
    const unsigned nb = mg_blocks(L.nn), nbt = mg_blocks((long long)N * L.nn);
    const int nt = N * L.nn;
    MG_LAUNCH(N, es_load_kernel, dim3(nb), MG_THREADS, st, L, o.F, o.V, U);
    MG_LAUNCH(N, es_init_kernel, dim3(nb), MG_THREADS, st, L, o.V, (const double*)o.V.x, f, o.V.r, o.V.z, jac);
    LSM_HIP(h, hipGetLastError());
    const int r1 = mg_iterate(h, o, max_iters, st, [&](int) {
        if (!jac) mg_vcycle(o, o.V.r, st);
        hipLaunchKernelGGL(es_dir_kernel<>, dim3(nbt), dim3(MG_THREADS), 0, st, nt, o.V);
        MG_LAUNCH(N, es_k1_kernel, dim3(nb), MG_THREADS, st, L, (const double*)o.V.p, o.V.q, o.partial.p, o.st.p);
        if (jac) hipLaunchKernelGGL(mg_k2_kernel<1>, dim3(nbt), dim3(MG_THREADS), 0, st, L.D, nt, (MgVec)o.V, (const double*)o.V.p);
        else hipLaunchKernelGGL(mg_k2_kernel<0>, dim3(nbt), dim3(MG_THREADS), 0, st, L.D, nt, (MgVec)o.V, (const double*)o.V.p);
    });
    if (r1 != LSM_OK) return r1;
    const int r2 = mg_report(h, o, "lsm_elastic_solve", rtol, iters_out, relres_out);
    if (r2 != LSM_OK) return r2;
    MG_LAUNCH(N, es_store_kernel, dim3(nb), MG_THREADS, st, L, o.F, (const double*)o.V.x, U);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(st));
    return LSM_OK;
}

// the batch workspace for K columns.  A larger one is built beside the old and takes its place only when every allocation succeeded
static int es_many_reserve(LsmHandle* h, ElasticObject& o, int K) {
    if (o.many && o.many->cols >= K) return LSM_OK;
    std::unique_ptr<MgSolver<EsLevel>> w(new MgSolver<EsLevel>());
    MgSolver<EsLevel>& M = *w;
    const int N = o.N, nl = (int)o.lev.size();
    M.N = N; M.precond = o.precond; M.cols = K; M.F = o.F;
    M.lev = o.lev;
    memcpy(M.co, o.co, sizeof(M.co));
    size_t nd = 0;
    for (int l = 0; l < nl; ++l) nd += (size_t)K * (size_t)N * (size_t)o.lev[l].nn * (size_t)(l ? 3 : 6);
    LSM_HIP(h, M.buf.alloc(nd * sizeof(double)));
    LSM_HIP(h, M.partial.alloc((size_t)K * 4 * MG_MAXB * sizeof(double)));
    LSM_HIP(h, M.st.alloc(K * sizeof(MgState)));
    LSM_HIP(h, M.h_st.alloc(K * sizeof(MgState)));
    M.rhs.assign(nl, nullptr); M.xa.assign(nl, nullptr); M.xb.assign(nl, nullptr);
    double* b = M.buf;
    for (int l = 0; l < nl; ++l) {
        const size_t m = (size_t)K * (size_t)N * (size_t)o.lev[l].nn;
        M.xa[l] = b; b += m;
        M.xb[l] = b; b += m;
        if (l) { M.rhs[l] = b; b += m; }
        else {
            M.V.x = b; b += m; M.V.r = b; b += m; M.V.q = b; b += m; M.V.p = b; b += m;
        }
    }
    M.V.z = o.precond == LSM_PRECOND_JACOBI ? M.xa[0] : M.xb[0];
    M.V.partial = M.partial;
    M.V.st = M.st;
    o.many = std::move(w);
    return LSM_OK;
}

// the K·N fields of a batched call: all given, no two the same
static bool es_fields_many(int N, int K, void* const* u, EsUMany& U) {
    memset(&U, 0, sizeof(U));
    if (!u) return false;
    for (int a = 0; a < K * N; ++a) {
        if (!u[a]) return false;
        for (int b = 0; b < a; ++b)
            if (u[b] == u[a]) return false;
        U.p[a / N][a % N] = u[a];
    }
    return true;
}

int lsm_elastic_solve_many(LsmElastic* s, int K, const double* f, void* const* u, double rtol, int max_iters, int* iters, double* relres, int* status,
                           void* stream) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    ElasticObject& o = *s->o;
    EsUMany U;
    if (K < 1 || K > LSM_ELASTIC_MAXCOLS) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_solve_many: K must be 1 ... LSM_ELASTIC_MAXCOLS (8)");
    if (!f || !iters || !relres || !status || !es_fields_many(o.N, K, u, U))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_solve_many: f, the K·N distinct fields of u and the three result arrays must be given");
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_solve_many: rtol must be positive and max_iters at least 1");
    const int N = o.N;
    const EsLevel& L = o.lev[0];
    const int jac = o.precond == LSM_PRECOND_JACOBI;
    (void)hipSetDevice(h->device);
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    const int ra = es_many_reserve(h, o, K);
    if (ra != LSM_OK) return ra;
    MgSolver<EsLevel>& M = *o.many;
    const int r0 = mg_reset(h, M, rtol, max_iters, st, K);
    if (r0 != LSM_OK) return r0;
    const unsigned nb = mg_blocks(L.nn), nbt = mg_blocks((long long)N * L.nn), nz = (unsigned)K;
    const int nt = N * L.nn;
    MG_LAUNCH2(N, es_load_kernel, EsUMany, dim3(nb, 1, nz), MG_THREADS, st, L, o.F, M.V, U);
    MG_LAUNCH2(N, es_init_kernel, 1, dim3(nb, 1, nz), MG_THREADS, st, L, M.V, (const double*)M.V.x, f, M.V.r, M.V.z, jac);
    LSM_HIP(h, hipGetLastError());
    const int r1 = mg_iterate(h, M, max_iters, st, [&](int) {
        if (!jac) mg_vcycle<1>(M, M.V.r, st, K);
        hipLaunchKernelGGL(es_dir_kernel<1>, dim3(nbt, 1, nz), dim3(MG_THREADS), 0, st, nt, M.V);
        MG_LAUNCH2(N, es_k1_kernel, 1, dim3(nb, 1, nz), MG_THREADS, st, L, (const double*)M.V.p, M.V.q, M.partial.p, M.st.p);
        if (jac) hipLaunchKernelGGL((mg_k2_kernel<1, 1>), dim3(nbt, 1, nz), dim3(MG_THREADS), 0, st, L.D, nt, (MgVec)M.V, (const double*)M.V.p);
        else hipLaunchKernelGGL((mg_k2_kernel<0, 1>), dim3(nbt, 1, nz), dim3(MG_THREADS), 0, st, L.D, nt, (MgVec)M.V, (const double*)M.V.p);
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
    if (bad >= 0) return mg_report(h, M, "lsm_elastic_solve_many", rtol, nullptr, nullptr, bad_input >= 0 ? bad_input : bad);
    M.last_iters = 0;
    for (int k = 0; k < K; ++k) M.last_iters = std::max(M.last_iters, iters[k]);
    MG_LAUNCH2(N, es_store_kernel, EsUMany, dim3(nb, 1, nz), MG_THREADS, st, L, o.F, (const double*)M.V.x, U);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipStreamSynchronize(st));
    return LSM_OK;
}

int lsm_elastic_energy_many(LsmElastic* s, int K, void* const* u, const double* w, void* e_out) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    EsUMany U;
    EsW W;
    memset(&W, 0, sizeof(W));
    if (K < 1 || K > LSM_ELASTIC_MAXCOLS) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_energy_many: K must be 1 ... LSM_ELASTIC_MAXCOLS (8)");
    if (!w || !e_out || !es_fields_many(s->o->N, K, u, U))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_energy_many: the K·N distinct fields of u, w and e_out must be given");
    for (int a = 0; a < K * s->o->N; ++a)
        if (u[a] == e_out) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_energy_many: e_out must not be one of the inputs");
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(w[k])) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_energy_many: the weights must be finite");
        W.w[k] = w[k];
    }
    const EsLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, es_energy_many_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, h->stream, L, s->o->F, U, K, W, e_out);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_energy_mutual(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* v0, const void* v1, const void* v2, void* e_out) {
    if (!s) return LSM_ERR_INVALID;
    EsU U, V;
    if (!es_fields(s->o->N, u0, u1, u2, U) || !es_fields(s->o->N, v0, v1, v2, V) || !e_out)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_energy_mutual: the components of u, those of v and e_out must be given, distinct within u and within v");
    for (int i = 0; i < s->o->N; ++i)
        if (e_out == U.p[i] || e_out == V.p[i]) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_energy_mutual: e_out must not be one of the inputs");
    const EsLevel& L = s->o->lev[0];
    MG_LAUNCH(s->o->N, es_energy_mutual_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, s->o->F, U, V, e_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

void lsm_elastic_destroy(LsmElastic* s) {
    if (!s) return;
    delete s->o;
    delete s;
}

// ======================================================================================================================================
// elasticity_modes: the m ≤ 8 smallest eigenpairs of A x = λ M x on the free components, M the lumped mass of the ersatz density, by a
// locally optimal block preconditioned CG (LOBPCG) whose preconditioner is mg_vcycle (or 1/D).  include/lsm.h ("elasticity_modes") is
// the normative text, tests/_modes_ref.py restates it, DESIGN.md §7.19 has the measurements.
//
// The iteration, its block passes (em_resid, em_gram, em_update), the host's Rayleigh–Ritz and the workspace are lobpcg.h's, shared with
// elliptic_modes (lsm_elliptic.hip).  This file's own: the block apply (one es_apply per column), the stored mode and the sensitivity.
namespace lsm {

// ---- y = A x per column (blockIdx.y), the rows of fixed components zero; x is zero on the fixed components
template <int N>
__global__ void __launch_bounds__(MG_THREADS) em_apply_kernel(EsLevel L, const double* __restrict__ x, double* __restrict__ y) {
    const int nn = L.nn;
    x += (size_t)blockIdx.y * (size_t)N * nn;
    y += (size_t)blockIdx.y * (size_t)N * nn;
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double out[N];
        es_apply<N>(L, id, I, [&](int q, int, int, int, int j) { return x[j * nn + q]; }, out);
#pragma unroll
        for (int i = 0; i < N; ++i) y[i * nn + id] = L.fixed(id, i) ? 0.0 : out[i];
    }
}

// ---- mode k into the N fields: x·scale rounded once to the storage type, exact zeros on the fixed components; the ghosts stay
template <int N>
__global__ void __launch_bounds__(MG_THREADS) em_store_kernel(EsLevel L, MgField F, const double* __restrict__ x, double scale, EsU U) {
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
#pragma unroll
        for (int i = 0; i < N; ++i) st_val(U.p[i], at, F.f32, L.fixed(id, i) ? 0.0 : x[i * L.nn + id] * scale);
    }
}

// ---- g_I = e_I − (λ·ρ̄_I)·(Σ_i u_{I,i}², from +0, i ascending), u = the stored mode (x·scale rounded to the storage type).  e_I is
// es_energy_kernel's, the same operations in the same order on values read from x instead of fields; ρ̄_I = (Σ ρ_C, ascending from +0)/cells
template <int N>
__global__ void __launch_bounds__(MG_THREADS) em_sens_kernel(EsLevel L, MgField F, const double* __restrict__ x, double scale, double lam,
                                                             const double* __restrict__ rho, void* __restrict__ g_out) {
    constexpr int NC = 1 << N, R = NC * N;
    const double* __restrict__ K = L.K;
    const int nn = L.nn, s1 = L.n[0], s2 = N > 2 ? L.n[0] * L.n[1] : 0;
    MG_LOOP(id, nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double acc = 0.0, cnt = 0.0, rs = 0.0;
#pragma unroll 1
        for (int m = 0; m < NC; ++m) {
            bool in;
            const double E = es_cell<N>(L, I, m, in);
            if (!in) continue;
            bool in2;
            rs = rs + em_cell(L, rho, I, m, N, in2);
            const int c0 = id + ((m & 1) - 1) + (((m >> 1) & 1) - 1) * s1 + (N > 2 ? (((m >> 2) & 1) - 1) * s2 : 0);     // the cell's lowest corner
            double uc[R];
#pragma unroll
            for (int b = 0; b < NC; ++b) {
                const int o = (b & 1) + ((b >> 1) & 1) * s1 + (N > 2 ? ((b >> 2) & 1) * s2 : 0);
#pragma unroll
                for (int j = 0; j < N; ++j) uc[b * N + j] = em_round(x[j * nn + c0 + o] * scale, F.f32);
            }
            double q = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double t = 0.0;
#pragma unroll
                for (int s = 0; s < R; ++s) t = t + K[r * R + s] * uc[s];
                q = q + uc[r] * t;
            }
            acc = acc + E * q;
            cnt = cnt + 1.0;
        }
        double sq = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const double u = em_round(x[i * nn + id] * scale, F.f32);
            sq = sq + u * u;
        }
        st_val(g_out, mg_padded(F, I), F.f32, acc / cnt - (lam * (rs / cnt)) * sq);
    }
}

}  // namespace lsm

struct LsmModes { LsmElastic* e; ModesObject* o; };

int lsm_elastic_modes_create(LsmElastic* s, const void* phi, double level, double rho_in, double rho_out, const double* rho_cells, int m, LsmModes** out) {
    if (!s) return LSM_ERR_INVALID;
    LsmHandle* h = s->h;
    ElasticObject& eo = *s->o;
    if (!out) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_create: null argument");
    if (!phi && !rho_cells) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_create: give phi or the cell densities");
    if (m < 1 || m > EM_MAXM) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_create: m must be between 1 and 8");
    if (3LL * m > eo.nfree) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_create: 3·m exceeds the number of free components");
    if (!rho_cells && (!(rho_in > 0) || !std::isfinite(rho_in) || !(rho_out > 0) || !std::isfinite(rho_out)))
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_create: rho_in and rho_out must be finite and positive");
    if (!rho_cells && !std::isfinite(level)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_create: level must be finite");
    (void)hipSetDevice(h->device);
    std::unique_ptr<ModesObject> guard(new ModesObject());
    const int r = em_create(h, eo, *guard, "lsm_elastic_modes_create", phi, level, rho_in, rho_out, rho_cells, m);
    if (r != LSM_OK) return r;
    *out = new LsmModes{s, guard.release()};
    return LSM_OK;
}

int lsm_elastic_modes_mass(LsmModes* md, double* node_mass) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    if (!node_mass) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_mass: null argument");
    LSM_HIP(h, hipMemcpyAsync(node_mass, md->o->Mn, (size_t)md->e->o->lev[0].nn * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return LSM_OK;
}

int lsm_elastic_modes_solve(LsmModes* md, const double* x0, double rtol, int max_iters, double* lambda, double* relres, int* iters, int64_t stats[4]) {
    if (!md) return LSM_ERR_INVALID;
    ElasticObject& eo = *md->e->o;
    const EsLevel& L = eo.lev[0];
    const int N = eo.N;
    return em_solve(md->e->h, eo, *md->o, "lsm_elastic_modes_solve",
                    [&](int na, const double* x, double* y, hipStream_t st) { MG_LAUNCH(N, em_apply_kernel, dim3(mg_blocks(L.nn), na), MG_THREADS, st, L, x, y); }, x0, rtol,
                    max_iters, lambda, relres, iters, stats);
}

int lsm_elastic_modes_vectors(LsmModes* md, double* x_out) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    if (!x_out || !md->o->solved) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_vectors: null argument, or no solve has run");
    LSM_HIP(h, hipMemcpyAsync(x_out, md->o->B.base, (size_t)md->o->m * (size_t)md->o->nt * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return LSM_OK;
}

int lsm_elastic_modes_store(LsmModes* md, int k, void* u0, void* u1, void* u2) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    ElasticObject& eo = *md->e->o;
    ModesObject& o = *md->o;
    EsU U;
    if (!o.solved || k < 0 || k >= o.m) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_store: no such mode, or no solve has run");
    if (!es_fields(eo.N, u0, u1, u2, U)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_store: the N distinct fields of u must be given");
    const EsLevel& L = eo.lev[0];
    MG_LAUNCH(eo.N, em_store_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, h->stream, L, eo.F, (const double*)(o.B.base + (size_t)k * o.nt), em_scale(L, eo.N), U);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_modes_sensitivity(LsmModes* md, int k, void* g_out) {
    if (!md) return LSM_ERR_INVALID;
    LsmHandle* h = md->e->h;
    ElasticObject& eo = *md->e->o;
    ModesObject& o = *md->o;
    if (!o.solved || k < 0 || k >= o.m || !g_out) return lsm_fail(h, LSM_ERR_INVALID, "lsm_elastic_modes_sensitivity: no such mode, no solve has run, or a null field");
    const EsLevel& L = eo.lev[0];
    MG_LAUNCH(eo.N, em_sens_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, h->stream, L, eo.F, (const double*)(o.B.base + (size_t)k * o.nt), em_scale(L, eo.N), o.lam[k],
              (const double*)o.rho, g_out);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

void lsm_elastic_modes_destroy(LsmModes* md) {
    if (!md) return;
    delete md->o;
    delete md;
}

// ======================================================================================================================================
// Stress recovery: the cell-mean strain and stress of a displacement, the von Mises field, the p-norm aggregate J′ = Σ_C (s_C/sref)^p
// with its adjoint load ∂J′/∂u and the cell sensitivity E_C·∂J′/∂E_C.  include/lsm.h ("stress recovery") is the normative text,
// tests/_stress_ref.py restates it, DESIGN.md §7.20 has the kernels' compiler report.
//
// Every quantity is a function of a cell's 2^N·N corner displacements, so every pass is one thread per cell (x-contiguous, each u
// value loaded by the 2^N cells that share it, from the cache) that leaves what the nodes need in the object's scratch vectors —
// xa, xb, x, r, q, p of level 0 are one run of 6·N·nn doubles, which a solve overwrites before it reads — and then one thread per
// node that gathers from the ≤ 2^N cells around it, ascending, without atomics.  Recomputing the cells per node, as es_energy_kernel
// does, would load and compute 2^N times as much.  One pow per cell and pass.
namespace lsm {

struct SsMat { double lam, mu, c[3]; int strain; };     // c_j = (1/h_j)·2^−(N−1); strain: 2-D plane strain (ŝ_zz = λ·tr, else 0)
struct SsOut { void* p[6]; };

template <int N>
__device__ __forceinline__ void ss_cell_coords(const int n[3], int ci, int C[3]) {
    C[0] = ci % (n[0] - 1);
    const int r = ci / (n[0] - 1);
    C[1] = N > 2 ? r % (n[1] - 1) : r;
    C[2] = N > 2 ? r / (n[1] - 1) : 0;
}
// the cell's corner values of the N fields, uc[b·N + i], as fp64
template <int N>
__device__ __forceinline__ void ss_corners(const MgField& F, const EsU& U, const int C[3], double uc[(1 << N) * N]) {
    const long long c0 = mg_padded(F, C);
#pragma unroll
    for (int b = 0; b < (1 << N); ++b) {
        const long long o = (b & 1) + ((b >> 1) & 1) * F.s1 + (N > 2 ? ((b >> 2) & 1) * F.s2 : 0);
#pragma unroll
        for (int i = 0; i < N; ++i) uc[b * N + i] = ld_val(U.p[i], c0 + o, F.f32);
    }
}
// shear component k of the Voigt order is the pair (i, j), i < j: 2-D (0,1); 3-D (1,2), (0,2), (0,1)
template <int N>
__device__ __forceinline__ constexpr int ss_pi(int k) { return N == 2 ? 0 : k == 0 ? 1 : 0; }
template <int N>
__device__ __forceinline__ constexpr int ss_pj(int k) { return N == 2 ? 1 : k == 2 ? 1 : 2; }

// the cell-mean gradient G_ij = d_ij·c_j, the strain e (Voigt), the unit normal stresses sn (the third is ŝ_zz in 2-D) and shears tau
template <int N>
__device__ __forceinline__ void ss_unit(const double uc[(1 << N) * N], const SsMat& P, double e[N * (N + 1) / 2], double sn[3], double tau[N == 2 ? 1 : 3]) {
    double G[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double d = 0.0;
#pragma unroll
            for (int b = 0; b < (1 << N); ++b) d = d + (((b >> j) & 1) ? uc[b * N + i] : -uc[b * N + i]);
            G[i][j] = d * P.c[j];
        }
    double tr = G[0][0] + G[1][1];
    if (N > 2) tr = tr + G[N - 1][N - 1];
    const double lt = P.lam * tr, mu2 = 2.0 * P.mu;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        e[i] = G[i][i];
        sn[i] = lt + mu2 * G[i][i];
    }
    if (N == 2) sn[2] = P.strain ? lt : 0.0;
#pragma unroll
    for (int k = 0; k < (N == 2 ? 1 : 3); ++k) {
        e[N + k] = G[ss_pi<N>(k)][ss_pj<N>(k)] + G[ss_pj<N>(k)][ss_pi<N>(k)];
        tau[k] = P.mu * e[N + k];
    }
}
// v2 = 0.5·(((a−b)² + (b−c)²) + (c−a)²) + 3·Σ τ̂²
template <int N>
__device__ __forceinline__ double ss_v2(const double sn[3], const double tau[N == 2 ? 1 : 3]) {
    const double ab = sn[0] - sn[1], bc = sn[1] - sn[2], ca = sn[2] - sn[0];
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < (N == 2 ? 1 : 3); ++k) q = q + tau[k] * tau[k];
    return 0.5 * ((ab * ab + bc * bc) + ca * ca) + 3.0 * q;
}

// ---- the cell arrays, component-major: the strain, the stress E_C·(ŝ, τ̂), or s_C = E_C·sqrt(v2)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) ss_cells_kernel(EsLevel L, MgField F, EsU U, SsMat P, int what, int nc, double* __restrict__ out) {
    constexpr int M = N * (N + 1) / 2;
    MG_LOOP(ci, nc) {
        int C[3];
        ss_cell_coords<N>(L.n, ci, C);
        double uc[(1 << N) * N], e[M], sn[3], tau[M - N];
        ss_corners<N>(F, U, C, uc);
        ss_unit<N>(uc, P, e, sn, tau);
        if (what == LSM_STRESS_STRAIN) {
#pragma unroll
            for (int k = 0; k < M; ++k) out[(size_t)k * nc + ci] = e[k];
        } else if (what == LSM_STRESS_STRESS) {
            const double E = L.E[ci];
#pragma unroll
            for (int k = 0; k < N; ++k) out[(size_t)k * nc + ci] = E * sn[k];
#pragma unroll
            for (int k = 0; k < M - N; ++k) out[(size_t)(N + k) * nc + ci] = E * tau[k];
        } else {
            out[ci] = L.E[ci] * sqrt(ss_v2<N>(sn, tau));
        }
    }
}

// the existing cells around node I, ascending m: their indices and their number
template <int N>
__device__ __forceinline__ double ss_around(const EsLevel& L, const int I[3], int ci[1 << N], bool in[1 << N]) {
    double cnt = 0.0;
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) {
        int C[3] = {0, 0, 0};
        in[m] = true;
#pragma unroll
        for (int d = 0; d < N; ++d) {
            C[d] = I[d] - 1 + ((m >> d) & 1);
            in[m] = in[m] && C[d] >= 0 && C[d] < L.n[d] - 1;
        }
        ci[m] = in[m] ? mg_cell_index<N>(L.n, C) : 0;
        if (in[m]) cnt = cnt + 1.0;
    }
    return cnt;
}

// ---- node fields from ncomp cell arrays: (scale·(Σ over the existing cells, ascending, from +0))/(their number), rounded once;
// scale = 1 for the plain fields, which changes no bit
template <int N>
__global__ void __launch_bounds__(MG_THREADS) ss_gather_kernel(EsLevel L, MgField F, const double* __restrict__ cell, int nc, int ncomp, double scale, SsOut O) {
    MG_LOOP(id, L.nn) {
        int I[3], ci[1 << N];
        bool in[1 << N];
        mg_coords<N>(L.n, id, I);
        const double cnt = ss_around<N>(L, I, ci, in);
        const long long at = mg_padded(F, I);
        for (int k = 0; k < ncomp; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < (1 << N); ++m)
                if (in[m]) acc = acc + cell[(size_t)k * nc + ci[m]];
            st_val(O.p[k], at, F.f32, (scale * acc) / cnt);
        }
    }
}

// ---- J′ = Σ_C pow(s_C/sref, p) in workgroup order and smax = max_C s_C, in one pass: out[0], out[1].  The workgroup's maximum goes
// into the second gridDim.x words of partial before block_reduce_ordered publishes the workgroup's sum, so the last workgroup finds
// both behind its acquire.  The maximum drops NaN; a NaN s_C makes J′ NaN, and smax is then set to it.
template <int N>
__global__ void __launch_bounds__(MG_THREADS) ss_norm_kernel(EsLevel L, MgField F, EsU U, SsMat P, int nc, double p, double sref, double* partial,
                                                             unsigned* ticket, double* __restrict__ out) {
    constexpr int M = N * (N + 1) / 2;
    __shared__ double wm[MG_THREADS / 64];
    double red[1] = {0.0}, mx = 0.0;
    MG_LOOP(ci, nc) {
        int C[3];
        ss_cell_coords<N>(L.n, ci, C);
        double uc[(1 << N) * N], e[M], sn[3], tau[M - N];
        ss_corners<N>(F, U, C, uc);
        ss_unit<N>(uc, P, e, sn, tau);
        const double s = L.E[ci] * sqrt(ss_v2<N>(sn, tau));
        red[0] += pow(s / sref, p);
        mx = s > mx ? s : mx;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    mx = wave_max(mx);
    if (lane == 0) wm[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) partial[gridDim.x + blockIdx.x] = fmax(fmax(wm[0], wm[1]), fmax(wm[2], wm[3]));
    if (!block_reduce_ordered<1, MG_THREADS>(red, partial, ticket)) return;
    mx = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += blockDim.x) {
        const double v = partial[gridDim.x + b];
        mx = v > mx ? v : mx;
    }
    mx = wave_max(mx);
    __syncthreads();
    if (lane == 0) wm[wave] = mx;
    __syncthreads();
    if (threadIdx.x != 0) return;
    out[0] = red[0];
    out[1] = red[0] != red[0] ? red[0] : fmax(fmax(wm[0], wm[1]), fmax(wm[2], wm[3]));
}

// ---- the adjoint load's cell pass: w_C = p·(E_C/sref)²·pow(r_C, p−2) and Z (Voigt: Z_ii, then the shears 3μ·τ̂) into 1 + M cell arrays
template <int N>
__global__ void __launch_bounds__(MG_THREADS) ss_loadcell_kernel(EsLevel L, MgField F, EsU U, SsMat P, int nc, double p, double sref, double* __restrict__ cell) {
    constexpr int M = N * (N + 1) / 2;
    MG_LOOP(ci, nc) {
        int C[3];
        ss_cell_coords<N>(L.n, ci, C);
        double uc[(1 << N) * N], e[M], sn[3], tau[M - N];
        ss_corners<N>(F, U, C, uc);
        ss_unit<N>(uc, P, e, sn, tau);
        const double E = L.E[ci];
        const double r = (E * sqrt(ss_v2<N>(sn, tau))) / sref, es = E / sref;
        cell[ci] = (p * (es * es)) * pow(r, p - 2.0);
        const double m[3] = {sn[0] - 0.5 * (sn[1] + sn[2]), sn[1] - 0.5 * (sn[0] + sn[2]), sn[2] - 0.5 * (sn[0] + sn[1])};
        double sm = m[0] + m[1];
        if (N > 2 || P.strain) sm = sm + m[2];
        const double ls = P.lam * sm, mu2 = 2.0 * P.mu, mu3 = 3.0 * P.mu;
#pragma unroll
        for (int i = 0; i < N; ++i) cell[(size_t)(1 + i) * nc + ci] = ls + mu2 * m[i];
#pragma unroll
        for (int k = 0; k < M - N; ++k) cell[(size_t)(1 + N + k) * nc + ci] = mu3 * tau[k];
    }
}
// ---- f_{I,i} = g_{I,i}/m_I, g_{I,i} = Σ over the existing cells, ascending, from +0, of w_C·(Σ_j ±(c_j·Z_ij), j ascending from +0): + where I is
// on the cell's upper side along j (bit j of m clear)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) ss_loadnode_kernel(EsLevel L, SsMat P, const double* __restrict__ cell, int nc, double* __restrict__ f_out) {
    constexpr int M = N * (N + 1) / 2;
    MG_LOOP(id, L.nn) {
        int I[3], ci[1 << N];
        bool in[1 << N];
        mg_coords<N>(L.n, id, I);
        ss_around<N>(L, I, ci, in);
        double g[N];
#pragma unroll
        for (int i = 0; i < N; ++i) g[i] = 0.0;
#pragma unroll
        for (int m = 0; m < (1 << N); ++m) {
            if (!in[m]) continue;
            const double w = cell[ci[m]];
            double Z[N][N];
#pragma unroll
            for (int i = 0; i < N; ++i) Z[i][i] = cell[(size_t)(1 + i) * nc + ci[m]];
#pragma unroll
            for (int k = 0; k < M - N; ++k) Z[ss_pi<N>(k)][ss_pj<N>(k)] = Z[ss_pj<N>(k)][ss_pi<N>(k)] = cell[(size_t)(1 + N + k) * nc + ci[m]];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double inner = 0.0;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const double t = P.c[j] * Z[i][j];
                    inner = inner + (((m >> j) & 1) ? -t : t);
                }
                g[i] = g[i] + w * inner;
            }
        }
        const double mass = mg_mass<N>(L.n, I);
#pragma unroll
        for (int i = 0; i < N; ++i) f_out[(size_t)i * L.nn + id] = g[i] / mass;
    }
}

// ---- the sensitivity's cell pass: p·pow(r_C, p) − E_C·(Σ_r λ_r·(Σ_s K0[r,s]·u_s)), the bilinear form in es_energy_kernel's order
template <int N>
__global__ void __launch_bounds__(MG_THREADS) ss_senscell_kernel(EsLevel L, MgField F, EsU U, EsU A, SsMat P, int nc, double p, double sref, double* __restrict__ cell) {
    constexpr int NC = 1 << N, R = NC * N, M = N * (N + 1) / 2;
    const double* __restrict__ K = L.K;
    MG_LOOP(ci, nc) {
        int C[3];
        ss_cell_coords<N>(L.n, ci, C);
        double uc[R], e[M], sn[3], tau[M - N];
        ss_corners<N>(F, U, C, uc);
        ss_unit<N>(uc, P, e, sn, tau);
        const double E = L.E[ci];
        const double r = (E * sqrt(ss_v2<N>(sn, tau))) / sref;
        double ac[R];
        ss_corners<N>(F, A, C, ac);
        double q = 0.0;
#pragma unroll
        for (int a = 0; a < R; ++a) {
            double t = 0.0;
#pragma unroll
            for (int s = 0; s < R; ++s) t = t + K[a * R + s] * uc[s];
            q = q + ac[a] * t;
        }
        cell[ci] = p * pow(r, p) - E * q;
    }
}

static SsMat ss_mat(const ElasticObject& o) {
    SsMat P;
    P.lam = o.lam; P.mu = o.mu;
    P.strain = o.N == 2 && o.plane == LSM_PLANE_STRAIN;
    for (int d = 0; d < 3; ++d) P.c[d] = d < o.N ? (1.0 / o.lev[0].h[d]) * (o.N == 2 ? 0.5 : 0.25) : 0.0;
    return P;
}
static bool ss_power(double p, double sref) { return p >= 2.0 && p <= 64.0 && std::isfinite(sref) && sref > 0.0; }

}  // namespace lsm

int lsm_elastic_stress_cells(LsmElastic* s, const void* u0, const void* u1, const void* u2, int what, double* out) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U;
    if (what != LSM_STRESS_STRAIN && what != LSM_STRESS_STRESS && what != LSM_STRESS_VON_MISES)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress_cells: unknown quantity (LSM_STRESS_STRAIN, LSM_STRESS_STRESS or LSM_STRESS_VON_MISES)");
    if (!es_fields(o.N, u0, u1, u2, U) || !out || out == u0 || out == u1 || out == u2)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress_cells: the N distinct fields of u and an array of its own must be given");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    MG_LAUNCH(o.N, ss_cells_kernel, dim3(mg_blocks(nc)), MG_THREADS, s->h->stream, L, o.F, U, ss_mat(o), what, nc, out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_stress(LsmElastic* s, const void* u0, const void* u1, const void* u2, int what, void* o0, void* o1, void* o2, void* o3, void* o4, void* o5) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U;
    if (what != LSM_STRESS_STRAIN && what != LSM_STRESS_STRESS && what != LSM_STRESS_VON_MISES)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress: unknown quantity (LSM_STRESS_STRAIN, LSM_STRESS_STRESS or LSM_STRESS_VON_MISES)");
    const int ncomp = what == LSM_STRESS_VON_MISES ? 1 : o.N * (o.N + 1) / 2;
    SsOut O = {{o0, o1, o2, o3, o4, o5}};
    bool ok = es_fields(o.N, u0, u1, u2, U);
    for (int k = 0; k < ncomp; ++k) {
        ok = ok && O.p[k] && O.p[k] != u0 && O.p[k] != u1 && O.p[k] != u2;
        for (int l = 0; l < k; ++l) ok = ok && O.p[k] != O.p[l];
    }
    if (!ok) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress: the components of u and the output fields must be distinct fields");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    hipStream_t st = s->h->stream;
    double* cell = o.xa[0];      // ≤ 6·(cells) of the 6·N·nn scratch doubles
    MG_LAUNCH(o.N, ss_cells_kernel, dim3(mg_blocks(nc)), MG_THREADS, st, L, o.F, U, ss_mat(o), what, nc, cell);
    MG_LAUNCH(o.N, ss_gather_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, o.F, (const double*)cell, nc, ncomp, 1.0, O);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_stress_norm(LsmElastic* s, const void* u0, const void* u1, const void* u2, double p, double sref, double out[2]) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U;
    if (!out || !es_fields(o.N, u0, u1, u2, U)) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress_norm: the N distinct fields of u and out must be given");
    if (!ss_power(p, sref)) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress_norm: p must lie in [2, 64] and sref must be positive and finite");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    hipStream_t st = s->h->stream;
    (void)hipSetDevice(s->h->device);
    double* res = o.partial.p + 2 * MG_MAXB;      // the reduction uses 2·gridDim.x ≤ 2·MG_MAXB words of the 4·MG_MAXB
    MG_LAUNCH(o.N, ss_norm_kernel, dim3(mg_blocks(nc)), MG_THREADS, st, L, o.F, U, ss_mat(o), nc, p, sref, o.partial.p, &o.st.p->ticket[3], res);
    LSM_HIP(s->h, hipGetLastError());
    LSM_HIP(s->h, hipMemcpyAsync(out, res, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    LSM_HIP(s->h, hipStreamSynchronize(st));
    return LSM_OK;
}

int lsm_elastic_stress_load(LsmElastic* s, const void* u0, const void* u1, const void* u2, double p, double sref, double* f_out) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U;
    if (!f_out || !es_fields(o.N, u0, u1, u2, U) || f_out == u0 || f_out == u1 || f_out == u2)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress_load: the N distinct fields of u and an array of its own must be given");
    if (!ss_power(p, sref)) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress_load: p must lie in [2, 64] and sref must be positive and finite");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    hipStream_t st = s->h->stream;
    const SsMat P = ss_mat(o);
    double* cell = o.xa[0];      // 1 + N(N+1)/2 ≤ 7 cell arrays of the 6·N·nn scratch doubles
    MG_LAUNCH(o.N, ss_loadcell_kernel, dim3(mg_blocks(nc)), MG_THREADS, st, L, o.F, U, P, nc, p, sref, cell);
    MG_LAUNCH(o.N, ss_loadnode_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, P, (const double*)cell, nc, f_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_stress_sensitivity(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* l0, const void* l1, const void* l2, double p,
                                   double sref, double scale, void* g_out) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U, A;
    if (!es_fields(o.N, u0, u1, u2, U) || !es_fields(o.N, l0, l1, l2, A) || !g_out || g_out == u0 || g_out == u1 || g_out == u2 || g_out == l0 || g_out == l1 ||
        g_out == l2)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress_sensitivity: the components of u, those of the adjoint and g_out must be distinct fields");
    if (!ss_power(p, sref) || !std::isfinite(scale))
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_stress_sensitivity: p must lie in [2, 64], sref must be positive and finite, scale finite");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    hipStream_t st = s->h->stream;
    double* cell = o.xa[0];
    SsOut O = {{g_out, nullptr, nullptr, nullptr, nullptr, nullptr}};
    MG_LAUNCH(o.N, ss_senscell_kernel, dim3(mg_blocks(nc)), MG_THREADS, st, L, o.F, U, A, ss_mat(o), nc, p, sref, cell);
    MG_LAUNCH(o.N, ss_gather_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, o.F, (const double*)cell, nc, 1, scale, O);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

// ======================================================================================================================================
// Topological derivative of the compliance: what a small traction-free hole at a cell would cost per unit volume removed, from the
// cell strain and unit stress of the stress recovery.  include/lsm.h ("topological derivative") is the normative text,
// tests/_topo_ref.py restates it, DESIGN.md §7.21.  One thread per cell, then the stress recovery's gather for the node field.
namespace lsm {

struct TdMat { double a, b; };

// a, b of T_C = E_C·(a·w + b·(trs·tr)), from the material at E = 1, in fp64 on the host
static TdMat td_mat(const ElasticObject& o) {
    const double lam = o.lam, mu = o.mu;
    TdMat T;
    if (o.N == 2) {
        const double g = (lam + 2.0 * mu) / ((2.0 * mu) * (lam + mu));
        T.a = g * (4.0 * mu);
        T.b = g * (lam - mu);
    } else {
        const double g = (3.0 * (lam + 2.0 * mu)) / ((4.0 * mu) * (9.0 * lam + 14.0 * mu));
        T.a = g * (20.0 * mu);
        T.b = g * (3.0 * lam - 2.0 * mu);
    }
    return T;
}

template <int N>
__global__ void __launch_bounds__(MG_THREADS) td_cells_kernel(EsLevel L, MgField F, EsU U, SsMat P, TdMat T, int nc, double* __restrict__ out) {
    constexpr int M = N * (N + 1) / 2;
    MG_LOOP(ci, nc) {
        int C[3];
        ss_cell_coords<N>(L.n, ci, C);
        double uc[(1 << N) * N], e[M], sn[3], tau[M - N];
        ss_corners<N>(F, U, C, uc);
        ss_unit<N>(uc, P, e, sn, tau);
        double w = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) w = w + sn[i] * e[i];
#pragma unroll
        for (int k = 0; k < M - N; ++k) w = w + tau[k] * e[N + k];
        double tr = e[0] + e[1], trs = sn[0] + sn[1];      // the in-plane traces in 2-D, also for plane strain
        if (N > 2) {
            tr = tr + e[2];
            trs = trs + sn[2];
        }
        out[ci] = L.E[ci] * (T.a * w + T.b * (trs * tr));
    }
}

}  // namespace lsm

int lsm_elastic_topo_cells(LsmElastic* s, const void* u0, const void* u1, const void* u2, double* out) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U;
    if (!es_fields(o.N, u0, u1, u2, U) || !out || out == u0 || out == u1 || out == u2)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_topo_cells: the N distinct fields of u and an array of its own must be given");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    MG_LAUNCH(o.N, td_cells_kernel, dim3(mg_blocks(nc)), MG_THREADS, s->h->stream, L, o.F, U, ss_mat(o), td_mat(o), nc, out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_topo(LsmElastic* s, const void* u0, const void* u1, const void* u2, void* o0) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U;
    if (!es_fields(o.N, u0, u1, u2, U) || !o0 || o0 == u0 || o0 == u1 || o0 == u2)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_topo: the components of u and the output field must be distinct fields");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    hipStream_t st = s->h->stream;
    double* cell = o.xa[0];      // one cell array of the 6·N·nn scratch doubles
    SsOut O = {{o0, nullptr, nullptr, nullptr, nullptr, nullptr}};
    MG_LAUNCH(o.N, td_cells_kernel, dim3(mg_blocks(nc)), MG_THREADS, st, L, o.F, U, ss_mat(o), td_mat(o), nc, cell);
    MG_LAUNCH(o.N, ss_gather_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, o.F, (const double*)cell, nc, 1, 1.0, O);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

// ======================================================================================================================================
// Thermoelastic coupling: a temperature field as a load on the structure, the stress with the thermal strain taken off, the elastic
// adjoint carried back into the heat problem, and the sensitivity of l·u to the cell moduli with the thermal load in it.
// include/lsm.h ("thermoelastic coupling") is the normative text, tests/_thermo_ref.py restates it, DESIGN.md §7.29.  The setting, SsMat,
// the gather rule and the launch caps are the stress recovery's.
//
// The load, the source and the sensitivity are node-owned gathers in one launch each, as es_energy_mutual_kernel is: a thread forms θ,
// tr and q of its ≤ 2^N cells from its 3^N neighbourhood, cell by cell in ascending m, without atomics and without a cell array.  The
// stress pair is the stress recovery's two passes with t_C taken off the normal unit stresses.
namespace lsm {

// β = 3λ + 2μ (3-D, plane strain) or 2λ + 2μ (plane stress); alpha: the scalar expansion coefficient, used where cells == NULL
struct ThMat { double beta, alpha, tref; const double* cells; };

static ThMat th_mat(const ElasticObject& o, double t_ref, double alpha, const double* alpha_cells) {
    ThMat H;
    H.beta = (o.N == 2 && o.plane == LSM_PLANE_STRESS ? 2.0 : 3.0) * o.lam + 2.0 * o.mu;
    H.alpha = alpha; H.tref = t_ref; H.cells = alpha_cells;
    return H;
}

// the padded offset of the lowest corner of cell m around the node at `at`, and of corner b from there
template <int N>
__device__ __forceinline__ long long th_cell0(const MgField& F, long long at, int m) {
    return at + ((m & 1) - 1) + (((m >> 1) & 1) - 1) * F.s1 + (N > 2 ? (((m >> 2) & 1) - 1) * F.s2 : 0);
}
template <int N>
__device__ __forceinline__ long long th_corner(const MgField& F, int b) {
    return (b & 1) + ((b >> 1) & 1) * F.s1 + (N > 2 ? ((b >> 2) & 1) * F.s2 : 0);
}
// t_C = ab_C·θ_C, ab_C = α_C·β, θ_C = (Σ_b T_b, b ascending from +0)·2^−N − t_ref; c0: the cell's lowest corner
template <int N>
__device__ __forceinline__ double th_unit(const MgField& F, const void* __restrict__ T, long long c0, int ci, const ThMat& H) {
    double sum = 0.0;
#pragma unroll
    for (int b = 0; b < (1 << N); ++b) sum = sum + ld_val(T, c0 + th_corner<N>(F, b), F.f32);
    const double theta = sum * (N == 2 ? 0.25 : 0.125) - H.tref;
    const double ab = (H.cells ? H.cells[ci] : H.alpha) * H.beta;
    return ab * theta;
}
// tr_C(v) = G_00 + G_11 (+ G_22) of the corner values vc[b·N + i], formed as ss_unit forms it
template <int N>
__device__ __forceinline__ double th_trace(const double vc[(1 << N) * N], const SsMat& P) {
    double G[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double d = 0.0;
#pragma unroll
        for (int b = 0; b < (1 << N); ++b) d = d + (((b >> i) & 1) ? vc[b * N + i] : -vc[b * N + i]);
        G[i] = d * P.c[i];
    }
    double tr = G[0] + G[1];
    if (N > 2) tr = tr + G[N - 1];
    return tr;
}

// ---- f_{I,i} = b_{I,i}/m_I, b_{I,i} = Σ over the existing cells, ascending, from +0, of ±(c_i·g_C), g_C = E_C·t_C: + where I is on the cell's
// upper side along i (bit i of m clear)
template <int N>
__global__ void __launch_bounds__(MG_THREADS) th_load_kernel(EsLevel L, MgField F, const void* __restrict__ T, SsMat P, ThMat H, double* __restrict__ f_out) {
    MG_LOOP(id, L.nn) {
        int I[3], ci[1 << N];
        bool in[1 << N];
        mg_coords<N>(L.n, id, I);
        ss_around<N>(L, I, ci, in);
        const long long at = mg_padded(F, I);
        double b[N];
#pragma unroll
        for (int i = 0; i < N; ++i) b[i] = 0.0;
#pragma unroll
        for (int m = 0; m < (1 << N); ++m) {
            if (!in[m]) continue;
            const double g = L.E[ci[m]] * th_unit<N>(F, T, th_cell0<N>(F, at, m), ci[m], H);
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const double t = P.c[i] * g;
                b[i] = b[i] + (((m >> i) & 1) ? -t : t);
            }
        }
        const double mass = mg_mass<N>(L.n, I);
#pragma unroll
        for (int i = 0; i < N; ++i) f_out[(size_t)i * L.nn + id] = b[i] / mass;
    }
}

// ---- the stress recovery's cell arrays with t_C off every normal unit stress (the out-of-plane one of plane strain included; plane
// stress keeps its 0): the stress E_C·(ŝ − t, τ̂) or s_C = E_C·sqrt(v2) of those values
template <int N>
__global__ void __launch_bounds__(MG_THREADS) th_cells_kernel(EsLevel L, MgField F, EsU U, const void* __restrict__ T, SsMat P, ThMat H, int what, int nc,
                                                              double* __restrict__ out) {
    constexpr int M = N * (N + 1) / 2;
    MG_LOOP(ci, nc) {
        int C[3];
        ss_cell_coords<N>(L.n, ci, C);
        double uc[(1 << N) * N], e[M], sn[3], tau[M - N];
        ss_corners<N>(F, U, C, uc);
        ss_unit<N>(uc, P, e, sn, tau);
        const double t = th_unit<N>(F, T, mg_padded(F, C), ci, H);
#pragma unroll
        for (int k = 0; k < N; ++k) sn[k] = sn[k] - t;
        if (N == 2 && P.strain) sn[2] = sn[2] - t;
        const double E = L.E[ci];
        if (what == LSM_STRESS_STRESS) {
#pragma unroll
            for (int k = 0; k < N; ++k) out[(size_t)k * nc + ci] = E * sn[k];
#pragma unroll
            for (int k = 0; k < M - N; ++k) out[(size_t)(N + k) * nc + ci] = E * tau[k];
        } else {
            out[ci] = E * sqrt(ss_v2<N>(sn, tau));
        }
    }
}

// ---- q_I = (Σ over the existing cells, ascending, from +0, of E_C·(ab_C·tr_C(v)))/(their number), nn fp64
template <int N>
__global__ void __launch_bounds__(MG_THREADS) th_source_kernel(EsLevel L, MgField F, EsU V, SsMat P, ThMat H, double* __restrict__ q_out) {
    constexpr int NC = 1 << N, R = NC * N;
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
        double acc = 0.0, cnt = 0.0;
#pragma unroll 1
        for (int m = 0; m < NC; ++m) {
            bool in;
            const double E = es_cell<N>(L, I, m, in);
            if (!in) continue;
            int C[3] = {0, 0, 0};
#pragma unroll
            for (int d = 0; d < N; ++d) C[d] = I[d] - 1 + ((m >> d) & 1);
            const long long c0 = th_cell0<N>(F, at, m);
            double vc[R];
#pragma unroll
            for (int b = 0; b < NC; ++b)
#pragma unroll
                for (int j = 0; j < N; ++j) vc[b * N + j] = ld_val(V.p[j], c0 + th_corner<N>(F, b), F.f32);
            const double ab = (H.cells ? H.cells[mg_cell_index<N>(L.n, C)] : H.alpha) * H.beta;
            acc = acc + E * (ab * th_trace<N>(vc, P));
            cnt = cnt + 1.0;
        }
        q_out[id] = acc / cnt;
    }
}

// ---- d_I = (Σ over the existing cells, ascending, from +0, of z_C)/(their number) − minus_I, z_C = E_C·(t_C·tr_C(v) − q_C), q_C the bilinear
// form in es_energy_mutual_kernel's order (u outside, v inside); minus == NULL: nothing is subtracted
template <int N>
__global__ void __launch_bounds__(MG_THREADS) th_sens_kernel(EsLevel L, MgField F, EsU U, EsU V, const void* __restrict__ T, SsMat P, ThMat H,
                                                             const void* __restrict__ minus, void* __restrict__ g_out) {
    constexpr int NC = 1 << N, R = NC * N;
    const double* __restrict__ K = L.K;
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        const long long at = mg_padded(F, I);
        double acc = 0.0, cnt = 0.0;
#pragma unroll 1
        for (int m = 0; m < NC; ++m) {
            bool in;
            const double E = es_cell<N>(L, I, m, in);
            if (!in) continue;
            int C[3] = {0, 0, 0};
#pragma unroll
            for (int d = 0; d < N; ++d) C[d] = I[d] - 1 + ((m >> d) & 1);
            const long long c0 = th_cell0<N>(F, at, m);
            double uc[R], vc[R];
#pragma unroll
            for (int b = 0; b < NC; ++b) {
                const long long o = th_corner<N>(F, b);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    uc[b * N + j] = ld_val(U.p[j], c0 + o, F.f32);
                    vc[b * N + j] = ld_val(V.p[j], c0 + o, F.f32);
                }
            }
            // the thermal term first: with it after the bilinear form the scheduler issues all of K0's scalar loads ahead of the block and
            // spills them to VGPR lanes (1169 in 3-D), which more than doubles the pass
            const double tt = th_unit<N>(F, T, c0, mg_cell_index<N>(L.n, C), H) * th_trace<N>(vc, P);
            double q = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double t = 0.0;
#pragma unroll
                for (int s = 0; s < R; ++s) t = t + K[r * R + s] * vc[s];
                q = q + uc[r] * t;
            }
            acc = acc + E * (tt - q);
            cnt = cnt + 1.0;
        }
        double d = acc / cnt;
        if (minus) d = d - ld_val(minus, at, F.f32);
        st_val(g_out, at, F.f32, d);
    }
}

// the refusals the five calls share: a temperature field, a finite reference temperature, a finite scalar alpha where it is used
static bool th_args(const void* T, double t_ref, double alpha, const double* alpha_cells) {
    return T && std::isfinite(t_ref) && (alpha_cells || std::isfinite(alpha));
}

}  // namespace lsm

int lsm_elastic_thermal_load(LsmElastic* s, const void* T, double t_ref, double alpha, const double* alpha_cells, double* f_out) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    if (!th_args(T, t_ref, alpha, alpha_cells)) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_load: T must be given, t_ref and a scalar alpha must be finite");
    if (!f_out || (const void*)f_out == T || (const void*)f_out == (const void*)alpha_cells)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_load: f_out must be an array of its own");
    const EsLevel& L = o.lev[0];
    MG_LAUNCH(o.N, th_load_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, o.F, T, ss_mat(o), th_mat(o, t_ref, alpha, alpha_cells), f_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_thermal_stress_cells(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* T, double t_ref, double alpha,
                                     const double* alpha_cells, int what, double* out) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U;
    if (what != LSM_STRESS_STRESS && what != LSM_STRESS_VON_MISES)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_stress_cells: unknown quantity (LSM_STRESS_STRESS or LSM_STRESS_VON_MISES: the total strain is lsm_elastic_stress_cells')");
    if (!th_args(T, t_ref, alpha, alpha_cells))
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_stress_cells: T must be given, t_ref and a scalar alpha must be finite");
    if (!es_fields(o.N, u0, u1, u2, U) || T == u0 || T == u1 || (o.N > 2 && T == u2) || !out || out == u0 || out == u1 || out == u2 || (const void*)out == T ||
        (const void*)out == (const void*)alpha_cells)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_stress_cells: the N fields of u and T must be distinct fields, out an array of its own");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    MG_LAUNCH(o.N, th_cells_kernel, dim3(mg_blocks(nc)), MG_THREADS, s->h->stream, L, o.F, U, T, ss_mat(o), th_mat(o, t_ref, alpha, alpha_cells), what, nc, out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_thermal_stress(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* T, double t_ref, double alpha, const double* alpha_cells,
                               int what, void* o0, void* o1, void* o2, void* o3, void* o4, void* o5) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U;
    if (what != LSM_STRESS_STRESS && what != LSM_STRESS_VON_MISES)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_stress: unknown quantity (LSM_STRESS_STRESS or LSM_STRESS_VON_MISES: the total strain is lsm_elastic_stress')");
    if (!th_args(T, t_ref, alpha, alpha_cells)) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_stress: T must be given, t_ref and a scalar alpha must be finite");
    const int ncomp = what == LSM_STRESS_VON_MISES ? 1 : o.N * (o.N + 1) / 2;
    SsOut O = {{o0, o1, o2, o3, o4, o5}};
    bool ok = es_fields(o.N, u0, u1, u2, U) && T != u0 && T != u1 && !(o.N > 2 && T == u2);
    for (int k = 0; k < ncomp; ++k) {
        ok = ok && O.p[k] && O.p[k] != u0 && O.p[k] != u1 && O.p[k] != u2 && O.p[k] != T && O.p[k] != (const void*)alpha_cells;
        for (int l = 0; l < k; ++l) ok = ok && O.p[k] != O.p[l];
    }
    if (!ok) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_stress: the components of u, T and the output fields must be distinct fields");
    const EsLevel& L = o.lev[0];
    const int nc = (int)mg_ncells(o.N, L);
    hipStream_t st = s->h->stream;
    double* cell = o.xa[0];      // ≤ 6·(cells) of the 6·N·nn scratch doubles
    MG_LAUNCH(o.N, th_cells_kernel, dim3(mg_blocks(nc)), MG_THREADS, st, L, o.F, U, T, ss_mat(o), th_mat(o, t_ref, alpha, alpha_cells), what, nc, cell);
    MG_LAUNCH(o.N, ss_gather_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, o.F, (const double*)cell, nc, ncomp, 1.0, O);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_thermal_source(LsmElastic* s, const void* v0, const void* v1, const void* v2, double alpha, const double* alpha_cells, double* q_out) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU V;
    if (!alpha_cells && !std::isfinite(alpha)) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_source: a scalar alpha must be finite");
    if (!es_fields(o.N, v0, v1, v2, V) || !q_out || q_out == v0 || q_out == v1 || q_out == v2 || (const void*)q_out == (const void*)alpha_cells)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_source: the N distinct fields of v and an array of its own must be given");
    const EsLevel& L = o.lev[0];
    MG_LAUNCH(o.N, th_source_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, o.F, V, ss_mat(o), th_mat(o, 0.0, alpha, alpha_cells), q_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}

int lsm_elastic_thermal_sensitivity(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* v0, const void* v1, const void* v2, const void* T,
                                    double t_ref, double alpha, const double* alpha_cells, const void* minus, void* g_out) {
    if (!s) return LSM_ERR_INVALID;
    ElasticObject& o = *s->o;
    EsU U, V;
    if (!th_args(T, t_ref, alpha, alpha_cells))
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_sensitivity: T must be given, t_ref and a scalar alpha must be finite");
    if (!es_fields(o.N, u0, u1, u2, U) || !es_fields(o.N, v0, v1, v2, V) || !g_out)
        return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_sensitivity: the components of u, those of v and g_out must be given, distinct within u and within v");
    bool ok = g_out != T && g_out != minus && g_out != (const void*)alpha_cells;
    for (int i = 0; i < o.N; ++i) ok = ok && g_out != U.p[i] && g_out != V.p[i] && T != U.p[i] && T != V.p[i];
    if (!ok) return lsm_fail(s->h, LSM_ERR_INVALID, "lsm_elastic_thermal_sensitivity: T must be none of u's or v's fields, g_out none of the inputs");
    const EsLevel& L = o.lev[0];
    MG_LAUNCH(o.N, th_sens_kernel, dim3(mg_blocks(L.nn)), MG_THREADS, s->h->stream, L, o.F, U, V, T, ss_mat(o), th_mat(o, t_ref, alpha, alpha_cells), minus, g_out);
    LSM_HIP(s->h, hipGetLastError());
    return LSM_OK;
}
