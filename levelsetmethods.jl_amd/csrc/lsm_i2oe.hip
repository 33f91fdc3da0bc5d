// lsm_i2oe.hip — SemiImplicitI2OE (src/timestepping.jl:204-426): one semi-implicit advection step, the global linear
// system solved on the device by unpreconditioned BiCGSTAB, matrix-free.
//
// The system.  With fac = Δt/(2·Πh), the face measure Π_{e≠d} h_e (1 in 1-D) and the face velocity v_f (½(v_p + v_q) for an
// ordinary neighbour q, v_p for a LinearExtrapolationBC ghost), every face f of dimension d carries ONE signed coefficient
//     c_f = fac · (area_d · v_f)
// and node p sees it as w = c on its lower face and w = -c on its upper face (the reference's fac·a_m, fac·a_p, :281-282).
// A side's ghost relation ghost(x) = α·x_p + β·x_idx (:371-412: interior and periodic α=0, β=1 towards the neighbour;
// NeumannBC α=0, β=1 towards p itself; LinearExtrapolationBC α=2, β=-1 towards the inward neighbour) turns the assembly of
// :276-362 into
//     (A x)_p = x_p + Σ_sides max(w,0) · (x_p - ghost(x))
//     rhs_p   = u_p - Σ_sides min(w,0) · (u_p - ghost(u))
// which is the reference's matrix with duplicates summed (a NeumannBC inflow entry lands on the diagonal and cancels).
// The diagonal stays implicit: the matvec reads the N face arrays and x.
//
// Storage.  Solver vectors are fp64 over the compact node index id = i0 + n0·(i1 + n1·i2); face array d has n_d + 1
// entries along d (face i between nodes i-1 and i; faces 0 and n_d belong to the boundary nodes only).  ϕ is read once
// (old values) and written once (the converged x), in the handle's storage type.
//
// Iteration (BiCGSTAB, r̂ = r₀), three kernels, each fused with the reductions it feeds; the scalars live on the device:
//   K1  p' = r + β(p - ω v) (p, v double-buffered: neighbours read the old ones)   v' = A p'      σ = r̂·v'     → α = ρ/σ
//   K2  s = r - α v                                                               t = A s        t·s, t·t, s·s → ω
//   K3  x += α p + ω s,  r = s - ω t                                                              r̂·r, r·r → ρ, β, done?
// Reductions are fp64: one partial per workgroup, the last workgroup to draw a ticket sums them in workgroup order
// (deterministic) and updates the scalars.  Every kernel returns at once when the device status is set (converged,
// breakdown, out of iterations), so the host enqueues iterations in chunks and reads the status once per chunk.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "lsm_handle.h"
#include "wave.h"

namespace lsm {

enum { I2_PER = 0, I2_NEU = 1, I2_LIN = 2 };
enum { I2_RUN = 0, I2_CONVERGED = 1, I2_MAXITER = 2, I2_BREAK_INPUT = -1, I2_BREAK_SIGMA = -2, I2_BREAK_OMEGA = -3, I2_BREAK_RHO = -4 };
static const int I2_THREADS = 256;
static const int I2_MAXB = 2048;

struct I2State {
    double rho, alpha, omega, beta, bb, rr, rtol2;
    int status, iters, max_iters, _pad;
    unsigned ticket[4];
};

struct I2Args {
    int ndim;
    unsigned n[3];
    unsigned nn;               // nodes
    unsigned cs[3];            // compact strides of the node index
    unsigned fm[3][3];         // extents of face array d
    unsigned fs[3];            // stride of dimension d inside face array d
    unsigned foff[3];          // offset of face array d in cf
    int kind[3][2];            // I2_* per dimension and side
    long long s1, s2, origin;  // padded layout of ϕ and of FIELD coefficients
    int gn[3];
    double lc[3], h[3];
    double fac, area[3];
    CoeffArgs vel;
    const void* phi_in;
    void* phi_out;
    int f32;
    double* cf;
    double *x, *r, *rh, *s, *t;
    double *p[2], *v[2];
    double* partial;           // 3 · gridDim.x
    I2State* st;
};

struct I2Rel { double a, b; int j; };

// ghost relation of side `side` (-1 / +1) of node i along a dimension of n nodes (src/timestepping.jl:371-412)
__device__ __forceinline__ I2Rel i2_rel(int i, int n, int side, int kind) {
    const int j = i + side;
    if (j >= 0 && j < n) return {0.0, 1.0, j};
    if (kind == I2_PER) return {0.0, 1.0, side < 0 ? n - 2 : 1};   // period n - 1 (_wrap_index_periodic)
    if (kind == I2_NEU) return {0.0, 1.0, i};                      // clamp to the node itself
    return {2.0, -1.0, side < 0 ? 1 : n - 2};                      // LinearExtrapolationBC: 1 + dist, -dist, inward neighbour
}

// component d of the node velocity (_eval_field, src/levelsetterms.jl:42-43; the conventions of include/lsm.h, LsmCoeff)
__device__ __forceinline__ double i2_vel(const I2Args& a, int d, const int I[3]) {
    const CoeffArgs& c = a.vel;
    if (c.kind == LSM_COEFF_CONST) return c.v[d];
    if (c.kind == LSM_COEFF_ROTATION) {
        if (d == 0) return -(c.v[0] * ((a.lc[1] + (double)I[1] * a.h[1]) - c.v[2]));
        if (d == 1) return c.v[0] * ((a.lc[0] + (double)I[0] * a.h[0]) - c.v[1]);
        return 0.0;
    }
    if (c.kind == LSM_COEFF_SEPARABLE) {
        const double* T = c.sep[d];
        double p = T[I[0]];
        if (a.ndim > 1) p = p * T[a.gn[0] + I[1]];
        if (a.ndim > 2) p = p * T[a.gn[0] + a.gn[1] + I[2]];
        return p * c.tfac;
    }
    return c.f[d][a.origin + I[0] + I[1] * a.s1 + I[2] * a.s2];
}

__device__ __forceinline__ void i2_coords(const I2Args& a, unsigned id, int I[3]) {
    I[0] = (int)(id % a.n[0]);
    const unsigned q = id / a.n[0];
    I[1] = (int)(q % a.n[1]);
    I[2] = (int)(q / a.n[1]);
}

__device__ __forceinline__ long long i2_padded(const I2Args& a, const int I[3]) { return a.origin + I[0] + I[1] * a.s1 + I[2] * a.s2; }

// Σ over the sides of node `id`: fn(w, rel, neighbour id) for every side (w = fac·a of the reference)
template <class F>
__device__ __forceinline__ void i2_sides(const I2Args& a, unsigned id, const int I[3], F fn) {
    for (int d = 0; d < a.ndim; ++d) {
        unsigned fid = 0;   // lower face of the node in face array d
        {
            unsigned s = 1;
            for (int e = 0; e < a.ndim; ++e) { fid += (unsigned)I[e] * s; s *= a.fm[d][e]; }
        }
        const double* cf = a.cf + a.foff[d];
        const double wm = cf[fid], wp = -cf[fid + a.fs[d]];
        const I2Rel rm = i2_rel(I[d], (int)a.n[d], -1, a.kind[d][0]);
        const I2Rel rp = i2_rel(I[d], (int)a.n[d], +1, a.kind[d][1]);
        fn(wm, rm, id + (unsigned)(rm.j - I[d]) * a.cs[d], d);
        fn(wp, rp, id + (unsigned)(rp.j - I[d]) * a.cs[d], d);
    }
}

// (A x)_p with x given as a function of the node id
template <class X>
__device__ __forceinline__ double i2_matvec(const I2Args& a, unsigned id, const int I[3], double xp, X xat) {
    double y = xp;
    i2_sides(a, id, I, [&](double w, const I2Rel& rl, unsigned q, int) {
        if (w > 0) y += w * (xp - (rl.a * xp + rl.b * xat(q)));
    });
    return y;
}

__device__ __forceinline__ bool i2_finite(double x) { return x - x == 0.0; }

// ---- assembly: the face coefficients of dimension d (one thread per face)
__global__ void __launch_bounds__(I2_THREADS) i2oe_faces_kernel(const I2Args a, int d) {
    const unsigned m0 = a.fm[d][0], m1 = a.fm[d][1], m2 = a.fm[d][2];
    const unsigned total = m0 * m1 * m2;
    const int n = (int)a.n[d];
    for (unsigned f = blockIdx.x * blockDim.x + threadIdx.x; f < total; f += gridDim.x * blockDim.x) {
        int F[3] = {(int)(f % m0), (int)((f / m0) % m1), (int)(f / (m0 * m1))};
        const int i = F[d];   // face between nodes i-1 and i
        double vf;
        if (i > 0 && i < n) {
            int P[3] = {F[0], F[1], F[2]};
            int Q[3] = {F[0], F[1], F[2]};
            P[d] = i - 1;
            vf = 0.5 * (i2_vel(a, d, P) + i2_vel(a, d, Q));
        } else {
            int P[3] = {F[0], F[1], F[2]};
            P[d] = i == 0 ? 0 : n - 1;
            const int kind = a.kind[d][i == 0 ? 0 : 1];
            const double vp = i2_vel(a, d, P);
            if (kind == I2_PER) {
                int Q[3] = {P[0], P[1], P[2]};
                Q[d] = i == 0 ? n - 2 : 1;
                vf = 0.5 * (vp + i2_vel(a, d, Q));
            } else if (kind == I2_NEU) {
                vf = 0.5 * (vp + vp);
            } else {
                vf = vp;
            }
        }
        a.cf[a.foff[d] + f] = a.fac * (a.area[d] * vf);
    }
}

// ---- rhs, r₀ = rhs - A u_old, x₀ = u_old, r̂ = r₀; ‖rhs‖², ‖r₀‖²
__global__ void __launch_bounds__(I2_THREADS) i2oe_init_kernel(const I2Args a) {
    double red[2] = {0.0, 0.0};
    for (unsigned id = blockIdx.x * blockDim.x + threadIdx.x; id < a.nn; id += gridDim.x * blockDim.x) {
        int I[3];
        i2_coords(a, id, I);
        const long long pp = i2_padded(a, I);
        const double up = ld_val(a.phi_in, pp, a.f32);
        double rhs = up, ax = up;
        i2_sides(a, id, I, [&](double w, const I2Rel& rl, unsigned, int d) {
            const long long stride = d == 0 ? 1 : (d == 1 ? a.s1 : a.s2);
            const double uq = ld_val(a.phi_in, pp + (long long)(rl.j - I[d]) * stride, a.f32);
            const double g = rl.a * up + rl.b * uq;
            if (w > 0) ax += w * (up - g);
            else if (w < 0) rhs -= w * (up - g);
            else if (w != w) rhs = w;   // NaN velocity: reported as a non-finite right-hand side
        });
        const double r = rhs - ax;
        a.x[id] = up;
        a.r[id] = r;
        a.rh[id] = r;
        a.p[0][id] = 0.0;
        a.v[0][id] = 0.0;
        red[0] += rhs * rhs;
        red[1] += r * r;
    }
    if (!block_reduce_ordered<2, I2_THREADS>(red, a.partial, &a.st->ticket[0]) || threadIdx.x != 0) return;
    I2State& S = *a.st;
    S.bb = red[0];
    S.rr = red[1];
    S.rho = red[1];
    S.alpha = 0.0; S.beta = 0.0; S.omega = 1.0;
    S.iters = 0;
    if (!i2_finite(red[0]) || !i2_finite(red[1])) S.status = I2_BREAK_INPUT;
    else if (red[1] <= S.rtol2 * red[0]) S.status = I2_CONVERGED;
    else S.status = I2_RUN;
}

// ---- K1: p' = r + β(p - ω v), v' = A p', σ = r̂·v', α = ρ/σ
__global__ void __launch_bounds__(I2_THREADS) i2oe_k1_kernel(const I2Args a, int par) {
    if (a.st->status != I2_RUN) return;
    const double beta = a.st->beta, omega = a.st->omega;
    const double* __restrict__ r = a.r;
    const double* __restrict__ po = a.p[par];
    const double* __restrict__ vo = a.v[par];
    double* __restrict__ pn = a.p[par ^ 1];
    double* __restrict__ vn = a.v[par ^ 1];
    auto pnew = [&](unsigned q) { return r[q] + beta * (po[q] - omega * vo[q]); };
    double red[1] = {0.0};
    for (unsigned id = blockIdx.x * blockDim.x + threadIdx.x; id < a.nn; id += gridDim.x * blockDim.x) {
        int I[3];
        i2_coords(a, id, I);
        const double pp = pnew(id);
        const double y = i2_matvec(a, id, I, pp, pnew);
        pn[id] = pp;
        vn[id] = y;
        red[0] += a.rh[id] * y;
    }
    if (!block_reduce_ordered<1, I2_THREADS>(red, a.partial, &a.st->ticket[1]) || threadIdx.x != 0) return;
    I2State& S = *a.st;
    const double alpha = S.rho / red[0];
    if (red[0] == 0.0 || !i2_finite(alpha)) { S.status = I2_BREAK_SIGMA; return; }
    S.alpha = alpha;
}

// ---- K2: s = r - α v, t = A s; ω = (t·s)/(t·t) (0 when s is already within the tolerance)
__global__ void __launch_bounds__(I2_THREADS) i2oe_k2_kernel(const I2Args a, int par) {
    if (a.st->status != I2_RUN) return;
    const double alpha = a.st->alpha;
    const double* __restrict__ r = a.r;
    const double* __restrict__ v = a.v[par ^ 1];
    auto sval = [&](unsigned q) { return r[q] - alpha * v[q]; };
    double red[3] = {0.0, 0.0, 0.0};
    for (unsigned id = blockIdx.x * blockDim.x + threadIdx.x; id < a.nn; id += gridDim.x * blockDim.x) {
        int I[3];
        i2_coords(a, id, I);
        const double s = sval(id);
        const double t = i2_matvec(a, id, I, s, sval);
        a.s[id] = s;
        a.t[id] = t;
        red[0] += t * s;
        red[1] += t * t;
        red[2] += s * s;
    }
    if (!block_reduce_ordered<3, I2_THREADS>(red, a.partial, &a.st->ticket[2]) || threadIdx.x != 0) return;
    I2State& S = *a.st;
    if (red[2] <= S.rtol2 * S.bb) { S.omega = 0.0; return; }   // x += α p solves it: K3 finds r = s converged
    const double omega = red[0] / red[1];
    if (red[1] == 0.0 || omega == 0.0 || !i2_finite(omega)) { S.status = I2_BREAK_OMEGA; return; }
    S.omega = omega;
}

// ---- K3: x += α p + ω s, r = s - ω t; ρ' = r̂·r, β = (ρ'/ρ)(α/ω), convergence on ‖r‖₂ ≤ rtol·‖rhs‖₂
__global__ void __launch_bounds__(I2_THREADS) i2oe_k3_kernel(const I2Args a, int par) {
    if (a.st->status != I2_RUN) return;
    const double alpha = a.st->alpha, omega = a.st->omega;
    const double* __restrict__ p = a.p[par ^ 1];
    double red[2] = {0.0, 0.0};
    for (unsigned id = blockIdx.x * blockDim.x + threadIdx.x; id < a.nn; id += gridDim.x * blockDim.x) {
        const double s = a.s[id];
        a.x[id] = a.x[id] + alpha * p[id] + omega * s;
        const double r = s - omega * a.t[id];
        a.r[id] = r;
        red[0] += a.rh[id] * r;
        red[1] += r * r;
    }
    if (!block_reduce_ordered<2, I2_THREADS>(red, a.partial, &a.st->ticket[3]) || threadIdx.x != 0) return;
    I2State& S = *a.st;
    S.iters += 1;
    S.rr = red[1];
    if (red[1] <= S.rtol2 * S.bb) { S.status = I2_CONVERGED; return; }
    if (!i2_finite(red[1]) || red[0] == 0.0 || !i2_finite(red[0])) { S.status = I2_BREAK_RHO; return; }
    S.beta = (red[0] / S.rho) * (alpha / omega);
    S.rho = red[0];
    if (S.iters >= S.max_iters) S.status = I2_MAXITER;
}

// ---- ϕ := x (rounded to the storage type)
__global__ void __launch_bounds__(I2_THREADS) i2oe_store_kernel(const I2Args a) {
    for (unsigned id = blockIdx.x * blockDim.x + threadIdx.x; id < a.nn; id += gridDim.x * blockDim.x) {
        int I[3];
        i2_coords(a, id, I);
        st_val(a.phi_out, i2_padded(a, I), a.f32, a.x[id]);
    }
}

struct I2oeWorkspace {
    DevBuf<double> buf;          // solver vectors + face arrays
    DevBuf<double> partial;      // 3 · I2_MAXB
    DevBuf<I2State> st;
    PinnedBuf<I2State> h_st;
    int last_iters = 0;          // iterations of the last solve: the size of the next call's first chunk
};

void i2oe_workspace_free(I2oeWorkspace* w) { delete w; }

}  // namespace lsm

using namespace lsm;

static const char* i2_bc_name(const LsmBc& b) {
    if (b.kind == LSM_BC_SYMMETRY) return "SymmetryBC";
    if (b.kind == LSM_BC_NONE) return "a slab interface";
    return "ExtrapolationBC";
}

int lsm_advance_i2oe(LsmHandle* h, const LsmTerm* term, void* phi, double tc, double dt, double rtol, int max_iters, int* iters_out,
                     double* rel_residual_out) {
    if (!h) return LSM_ERR_INVALID;
    if (!term || !phi) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_i2oe: null argument");
    if (h->comm) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_i2oe: SemiImplicitI2OE runs on a single device (a communicator is attached)");
    if (term->kind != LSM_TERM_ADVECTION) return lsm_fail(h, LSM_ERR_INVALID, "SemiImplicitI2OE requires exactly one AdvectionTerm");
    const int N = h->grid.ndim;
    for (int d = 0; d < N; ++d)
        if (h->nloc[d] < 3 || h->gn[d] < 3) return lsm_fail(h, LSM_ERR_INVALID, "SemiImplicitI2OE requires at least 3 grid nodes along each dimension");
    I2Args a;
    memset(&a, 0, sizeof(a));
    for (int d = 0; d < N; ++d)
        for (int s = 0; s < 2; ++s) {
            const LsmBc& b = h->bc[d][s];
            if (b.kind == LSM_BC_PERIODIC) a.kind[d][s] = I2_PER;
            else if (b.kind == LSM_BC_EXTRAPOLATION && b.degree == 0) a.kind[d][s] = I2_NEU;
            else if (b.kind == LSM_BC_EXTRAPOLATION && b.degree == 1) a.kind[d][s] = I2_LIN;
            else {
                std::string name = i2_bc_name(b);
                if (b.kind == LSM_BC_EXTRAPOLATION) name += "{" + std::to_string(b.degree) + "}";
                return lsm_fail(h, LSM_ERR_INVALID, "boundary condition " + name + " is not supported by SemiImplicitI2OE");
            }
        }
    const int ck = term->coeff.kind;
    if (ck != LSM_COEFF_CONST && ck != LSM_COEFF_ROTATION && ck != LSM_COEFF_SEPARABLE && ck != LSM_COEFF_FIELD)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_i2oe: unknown coefficient kind");
    if (ck == LSM_COEFF_SEPARABLE && term->coeff.time_kind != LSM_TIME_ONE && term->coeff.time_kind != LSM_TIME_COS)
        return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_i2oe: unknown time factor");
    for (int d = 0; d < N; ++d)
        if ((ck == LSM_COEFF_FIELD && !term->coeff.field[d]) || (ck == LSM_COEFF_SEPARABLE && !term->coeff.sep[d]))
            return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_i2oe: missing coefficient component");
    if (!(rtol > 0) || max_iters < 1) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_i2oe: rtol must be positive and max_iters at least 1");
    if (!(dt >= 0) || !std::isfinite(dt)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_i2oe: Δt must be finite and non-negative");

    // geometry (32-bit node and face indices)
    unsigned long long nn = 1;
    for (int d = 0; d < 3; ++d) nn *= (unsigned long long)(d < N ? h->nloc[d] : 1);
    unsigned long long nf_total = 0;
    for (int d = 0; d < N; ++d) nf_total += nn / (unsigned long long)h->nloc[d] * (unsigned long long)(h->nloc[d] + 1);
    if (nn + nf_total >= (1ull << 31)) return lsm_fail(h, LSM_ERR_INVALID, "lsm_advance_i2oe: grid too large (2^31 nodes and faces at most)");
    a.ndim = N;
    unsigned cs = 1, foff = 0;
    for (int d = 0; d < 3; ++d) {
        a.n[d] = d < N ? (unsigned)h->nloc[d] : 1u;
        a.gn[d] = h->gn[d];
        a.lc[d] = h->grid.lc[d];
        a.h[d] = h->h[d];
    }
    for (int d = 0; d < 3; ++d) { a.cs[d] = cs; cs *= a.n[d]; }
    a.nn = (unsigned)nn;
    for (int d = 0; d < N; ++d) {
        unsigned s = 1;
        for (int e = 0; e < 3; ++e) {
            a.fm[d][e] = a.n[e] + (e == d ? 1u : 0u);
            if (e == d) a.fs[d] = s;
            s *= a.fm[d][e];
        }
        a.foff[d] = foff;
        foff += s;
    }
    // fac = Δt / (2·Πh), face measure Π_{e≠d} h_e or 1 in 1-D (src/timestepping.jl:258-260,421-426)
    double mp = h->h[0];
    for (int d = 1; d < N; ++d) mp *= h->h[d];
    a.fac = dt / (2 * mp);
    for (int d = 0; d < N; ++d) {
        double ar = 1.0;
        bool first = true;
        for (int e = 0; e < N; ++e)
            if (e != d) { ar = first ? h->h[e] : ar * h->h[e]; first = false; }
        a.area[d] = N == 1 ? 1.0 : ar;
    }
    a.vel.kind = ck;
    for (int k = 0; k < 4; ++k) a.vel.v[k] = term->coeff.value[k];
    a.vel.tfac = ck == LSM_COEFF_SEPARABLE && term->coeff.time_kind == LSM_TIME_COS ? cos(M_PI * tc / term->coeff.time_param) : 1.0;
    for (int k = 0; k < 3; ++k) { a.vel.f[k] = (const double*)term->coeff.field[k]; a.vel.sep[k] = term->coeff.sep[k]; }
    a.s1 = h->lay.stride[1]; a.s2 = h->lay.stride[2]; a.origin = h->lay.origin;
    a.phi_in = phi;
    a.phi_out = phi;
    a.f32 = h->dtype == LSM_DTYPE_F32 ? 1 : 0;

    // workspace: x r r̂ s t p₀ p₁ v₀ v₁ + face arrays, owned by the handle (grow-only)
    (void)hipSetDevice(h->device);
    if (!h->i2oe_ws) h->i2oe_ws = new I2oeWorkspace();
    I2oeWorkspace& W = *h->i2oe_ws;
    const size_t need = 9 * (size_t)nn + (size_t)nf_total;
    if (W.buf.cap < need * sizeof(double)) {
        if (W.buf) LSM_HIP(h, hipStreamSynchronize(h->stream));
        LSM_HIP(h, W.buf.alloc(need * sizeof(double)));
    }
    if (!W.partial) LSM_HIP(h, W.partial.alloc(3 * I2_MAXB * sizeof(double)));
    if (!W.st) LSM_HIP(h, W.st.alloc(sizeof(I2State)));
    if (!W.h_st) LSM_HIP(h, W.h_st.alloc(sizeof(I2State)));
    double* b = W.buf;
    a.x = b; a.r = b + nn; a.rh = b + 2 * nn; a.s = b + 3 * nn; a.t = b + 4 * nn;
    a.p[0] = b + 5 * nn; a.p[1] = b + 6 * nn; a.v[0] = b + 7 * nn; a.v[1] = b + 8 * nn;
    a.cf = b + 9 * nn;
    a.partial = W.partial;
    a.st = W.st;

    I2State s0;
    memset(&s0, 0, sizeof(s0));
    s0.rtol2 = rtol * rtol;
    s0.max_iters = max_iters;
    hipStream_t st = h->stream;
    LSM_HIP(h, hipMemcpyAsync(W.st, &s0, sizeof(s0), hipMemcpyHostToDevice, st));
    const unsigned nb = (unsigned)std::min<unsigned long long>((nn + I2_THREADS - 1) / I2_THREADS, I2_MAXB);
    for (int d = 0; d < N; ++d) {
        const unsigned long long nf = nn / a.n[d] * (a.n[d] + 1);
        const unsigned fb = (unsigned)std::min<unsigned long long>((nf + I2_THREADS - 1) / I2_THREADS, 8192);
        hipLaunchKernelGGL(i2oe_faces_kernel, dim3(fb), dim3(I2_THREADS), 0, st, a, d);
    }
    hipLaunchKernelGGL(i2oe_init_kernel, dim3(nb), dim3(I2_THREADS), 0, st, a);
    LSM_HIP(h, hipGetLastError());

    // iterations in chunks: the first chunk is as long as the last solve took, then doubling
    int enq = 0;
    int chunk = std::max(4, W.last_iters + 1);
    for (;;) {
        const int k = std::min(chunk, max_iters - enq);
        for (int it = 0; it < k; ++it, ++enq) {
            const int par = enq & 1;
            hipLaunchKernelGGL(i2oe_k1_kernel, dim3(nb), dim3(I2_THREADS), 0, st, a, par);
            hipLaunchKernelGGL(i2oe_k2_kernel, dim3(nb), dim3(I2_THREADS), 0, st, a, par);
            hipLaunchKernelGGL(i2oe_k3_kernel, dim3(nb), dim3(I2_THREADS), 0, st, a, par);
        }
        LSM_HIP(h, hipGetLastError());
        LSM_HIP(h, hipMemcpyAsync(W.h_st, W.st, sizeof(I2State), hipMemcpyDeviceToHost, st));
        LSM_HIP(h, hipStreamSynchronize(st));
        if (W.h_st.p->status != I2_RUN || enq >= max_iters) break;
        chunk = std::min(2 * chunk, 64);
    }
    const I2State S = *W.h_st;
    const double rel = S.bb > 0 ? std::sqrt(S.rr / S.bb) : (S.rr == 0 ? 0.0 : std::sqrt(S.rr));
    if (iters_out) *iters_out = S.iters;
    if (rel_residual_out) *rel_residual_out = rel;
    W.last_iters = S.iters;
    if (S.status != I2_CONVERGED) {
        char msg[320];
        const char* why = S.status == I2_MAXITER || S.status == I2_RUN ? "no convergence within max_iters"
                          : S.status == I2_BREAK_INPUT ? "non-finite right-hand side or initial residual (NaN/Inf in ϕ or the velocity)"
                          : S.status == I2_BREAK_SIGMA ? "BiCGSTAB breakdown (r̂·v = 0 or non-finite α)"
                          : S.status == I2_BREAK_OMEGA ? "BiCGSTAB breakdown (ω = 0 or non-finite)"
                                                       : "BiCGSTAB breakdown (ρ = 0 or non-finite residual)";
        snprintf(msg, sizeof(msg), "SemiImplicitI2OE: %s: %d iterations, relative residual %.3e (rtol %.3e); ϕ is unchanged", why, S.iters,
                 rel, rtol);
        return lsm_fail(h, LSM_ERR_NOT_CONVERGED, msg);
    }
    hipLaunchKernelGGL(i2oe_store_kernel, dim3(nb), dim3(I2_THREADS), 0, st, a);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}
