// lobpcg.h — the locally optimal block preconditioned CG (LOBPCG) that elasticity_modes (lsm_elastic.hip) and elliptic_modes
// (lsm_elliptic.hip) share: the m ≤ 8 smallest eigenpairs of A x = λ M x on the free components of an mg_pcg.h operator, M a lumped
// node mass, the preconditioner one mg_vcycle (or 1/D).  include/lsm.h ("elasticity_modes") is the normative text of the iteration,
// tests/_modes_ref.py restates it, DESIGN.md §7.19 and §7.26 have the measurements.
//
// Blocks.  Six blocks of m columns of nt = comps·nn doubles in one allocation: X, W, P, A·X, A·W, A·P; column k of block b starts at
// (b·m + k)·nt.  W and P hold na ≤ m columns, in slots 0 … na−1: one per column of X that has not converged (soft locking).
// One iteration: em_resid (R = A·X − M·X·Λ into W's slots, the 2m norms) → the host picks the active columns → per active column one
// mg_vcycle on the residual's slot, its result copied into W's next slot → the operator's block apply (A·W, fixed rows zero) → em_gram
// (SᵀA S, SᵀM S, S = [X, W, P]) → the host's Rayleigh–Ritz (cyclic Jacobi) → em_update (X, P, A·X, A·P ← S·C, in place, row by row).
// The Gram pass forms 4×4 tiles of the upper triangle, one tile per blockIdx.y: 32 fp64 accumulators a thread (both matrices), plain
// multiply and add; each entry is summed over a thread's rows ascending, then by block_reduce_ordered.  The host mirrors the triangle.
//
// What an operator supplies: its MgSolver<Level> (Level::comps, fixed(id, comp), D, the V-cycle, the MgState) and a block apply
// "y_j = A x_j for na columns, the rows of fixed components zero" (em_solve's `apply`).  The kernels that read a Level are templates
// on it, as mg_pcg.h's are; the others are static: one copy per translation unit that includes this header.
#pragma once
#include <memory>

#include "el_cell.h"
#include "mg_pcg.h"

namespace lsm {

static const int EM_MAXM = 8, EM_TILE = 4, EM_MAXT = 21, EM_GRAMB = 512;
enum { EM_OUT_GRAM = 0, EM_OUT_NORM = EM_MAXT * 32, EM_OUT_N = EM_MAXT * 32 + 2 * EM_MAXM };

struct EmBlocks { double* base; long long nt; int m, na, np; };
struct EmTiles { unsigned char bi[EM_MAXT], bj[EM_MAXT]; };
struct EmLam { double v[EM_MAXM]; };

// column c of S = [X, W, P] (a = 0) or of A·S (a = 1)
__device__ __forceinline__ double* em_col(const EmBlocks& B, int c, int a) {
    const int b = c < B.m ? 0 : c < B.m + B.na ? 1 : 2;
    const int k = c - (b == 0 ? 0 : b == 1 ? B.m : B.m + B.na);
    return B.base + (size_t)((3 * a + b) * B.m + k) * (size_t)B.nt;
}
template <class Level>
__device__ __forceinline__ double em_cell(const Level& L, const double* __restrict__ c, const int I[3], int m, int N, bool& in) {
    int C[3] = {0, 0, 0};
    in = true;
    for (int d = 0; d < N; ++d) {
        C[d] = I[d] - 1 + ((m >> d) & 1);
        in = in && C[d] >= 0 && C[d] < L.n[d] - 1;
    }
    return in ? c[C[0] + (L.n[0] - 1) * (C[1] + (N > 2 ? (L.n[1] - 1) * C[2] : 0))] : 0.0;
}

// ---- the cell densities: el_cell.h's value with (ρ_in, ρ_out), or the caller's, checked; cnt[0]: non-finite ϕ, cnt[1]: ρ not finite and positive
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) em_rho_kernel(Level L, MgField F, const void* __restrict__ phi, double level, double rho_in, double rho_out,
                                                            double hmin, const double* __restrict__ given, double* __restrict__ rho, unsigned long long* cnt) {
    unsigned bad[2] = {0, 0};
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        if (phi && !mg_finite(ld_val(phi, mg_padded(F, I), F.f32))) ++bad[0];
        bool corner = true;
#pragma unroll
        for (int d = 0; d < N; ++d) corner = corner && I[d] < L.n[d] - 1;
        if (!corner) continue;
        const int ci = I[0] + (L.n[0] - 1) * (I[1] + (N > 2 ? (L.n[1] - 1) * I[2] : 0));
        const double v = given ? given[ci] : el_cell_from_phi<N>(phi, mg_padded(F, I), F.s1, F.s2, F.f32, level, rho_in, rho_out, hmin);
        if (!(v > 0.0) || !mg_finite(v)) ++bad[1];
        rho[ci] = v;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned v = wave_sum(bad[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&cnt[k], (unsigned long long)v);
    }
}
// ---- M_I = (Σ ρ_C over the existing cells around I, ascending, from +0)·2^−N
template <int N, class Level>
__global__ void __launch_bounds__(MG_THREADS) em_mass_kernel(Level L, const double* __restrict__ rho, double* __restrict__ Mn) {
    MG_LOOP(id, L.nn) {
        int I[3];
        mg_coords<N>(L.n, id, I);
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < (1 << N); ++m) {
            bool in;
            const double r = em_cell(L, rho, I, m, N, in);
            if (in) acc = acc + r;
        }
        Mn[id] = acc * (N == 2 ? 0.25 : 0.125);
    }
}

// ---- the default start: splitmix64 of the entry's linear index, its top 53 bits a double in [0, 1), mapped to (−1, 1); zero on fixed components.
// N: the components of a node
template <class Level>
__global__ void __launch_bounds__(MG_THREADS) em_init_kernel(Level L, int N, long long total, const double* __restrict__ x0, double* __restrict__ X) {
    const long long nt = (long long)N * L.nn;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long r = t % nt;
        const int i = (int)(r / L.nn), id = (int)(r % L.nn);
        double v;
        if (x0) v = x0[t];
        else {
            unsigned long long z = (unsigned long long)t + 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z = z ^ (z >> 31);
            v = 2.0 * ((double)(z >> 11) * 0x1p-53) - 1.0;
        }
        X[t] = L.fixed(id, i) ? 0.0 : v;
    }
}

// ---- R_k = A·X_k − λ_k·(M·X_k) into slot k of W, and ‖R_k‖², ‖M·X_k‖² for every k, in one pass
static __global__ void __launch_bounds__(MG_THREADS) em_resid_kernel(EmBlocks B, int nn, EmLam lam, const double* __restrict__ Mn, double* partial, unsigned* ticket,
                                                              double* __restrict__ out) {
    double red[2 * EM_MAXM];
#pragma unroll
    for (int k = 0; k < 2 * EM_MAXM; ++k) red[k] = 0.0;
    const size_t nt = (size_t)B.nt;
    const double* __restrict__ X = B.base;
    const double* __restrict__ AX = B.base + (size_t)3 * B.m * nt;
    double* __restrict__ W = B.base + (size_t)B.m * nt;
    MG_LOOP(t, (int)B.nt) {
        const double mass = Mn[t % nn];
#pragma unroll
        for (int k = 0; k < EM_MAXM; ++k) {
            if (k < B.m) {
                const double mx = mass * X[k * nt + t];
                const double r = AX[k * nt + t] - lam.v[k] * mx;
                W[k * nt + t] = r;
                red[2 * k] += r * r;
                red[2 * k + 1] += mx * mx;
            }
        }
    }
    if (!block_reduce_ordered<2 * EM_MAXM, MG_THREADS>(red, partial, ticket) || threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < 2 * EM_MAXM; ++k) out[k] = red[k];
}

// ---- dst = src (the V-cycle's result into its slot), or src/D on the free components (the diagonal preconditioner); elementwise, so src may be dst
template <class Level>
__global__ void __launch_bounds__(MG_THREADS) em_precond_kernel(Level L, int nt, const double* src, const double* __restrict__ D, double* dst) {
    MG_LOOP(t, nt) dst[t] = D ? (L.fixed(t % L.nn, t / L.nn) ? 0.0 : src[t] / D[t]) : src[t];
}

// ---- tile (bi, bj) of SᵀA S and SᵀM S: entry (a, b) of the tile is Σ_t S_{4bi+a}[t]·(A S)_{4bj+b}[t] and Σ_t S_{4bi+a}[t]·(M[t]·S_{4bj+b}[t])
static __global__ void __launch_bounds__(MG_THREADS) em_gram_kernel(EmBlocks B, int nn, EmTiles tiles, const double* __restrict__ Mn, double* partial, unsigned* tickets,
                                                             double* __restrict__ out) {
    const int T = blockIdx.y, bi = tiles.bi[T], bj = tiles.bj[T], q = B.m + B.na + B.np;
    const double *si[EM_TILE], *sj[EM_TILE], *aj[EM_TILE];
    bool vi[EM_TILE], vj[EM_TILE];
#pragma unroll
    for (int e = 0; e < EM_TILE; ++e) {
        vi[e] = EM_TILE * bi + e < q;
        vj[e] = EM_TILE * bj + e < q;
        si[e] = em_col(B, vi[e] ? EM_TILE * bi + e : 0, 0);
        sj[e] = em_col(B, vj[e] ? EM_TILE * bj + e : 0, 0);
        aj[e] = em_col(B, vj[e] ? EM_TILE * bj + e : 0, 1);
    }
    double red[2 * EM_TILE * EM_TILE];
#pragma unroll
    for (int k = 0; k < 2 * EM_TILE * EM_TILE; ++k) red[k] = 0.0;
    MG_LOOP(t, (int)B.nt) {
        const double mass = Mn[t % nn];
        double xi[EM_TILE], mj[EM_TILE], yj[EM_TILE];
#pragma unroll
        for (int e = 0; e < EM_TILE; ++e) {
            xi[e] = vi[e] ? si[e][t] : 0.0;
            mj[e] = vj[e] ? mass * sj[e][t] : 0.0;
            yj[e] = vj[e] ? aj[e][t] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < EM_TILE; ++a)
#pragma unroll
            for (int b = 0; b < EM_TILE; ++b) {
                red[a * EM_TILE + b] += xi[a] * yj[b];
                red[EM_TILE * EM_TILE + a * EM_TILE + b] += xi[a] * mj[b];
            }
    }
    if (!block_reduce_ordered<2 * EM_TILE * EM_TILE, MG_THREADS>(red, partial + (size_t)T * 2 * EM_TILE * EM_TILE * gridDim.x, &tickets[T]) || threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < 2 * EM_TILE * EM_TILE; ++k) out[T * 2 * EM_TILE * EM_TILE + k] = red[k];
}

// ---- X, P ← S·C (blockIdx.y = 0) and A·X, A·P ← (A S)·C (1), row by row in place.  C: two matrices of 24 rows × 8 columns, row-major,
// the rows in slot order (X's 8 slots, W's, P's; zero where there is no column): Cx for the new X, Cp for the new P
static __global__ void __launch_bounds__(MG_THREADS) em_update_kernel(EmBlocks B, const double* __restrict__ C) {
    const size_t nt = (size_t)B.nt;
    double* __restrict__ base = B.base + (size_t)blockIdx.y * 3 * B.m * nt;
    const int cnt[3] = {B.m, B.na, B.np};
    MG_LOOP(t, (int)B.nt) {
        double s[3 * EM_MAXM];
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int k = 0; k < EM_MAXM; ++k) s[b * EM_MAXM + k] = k < cnt[b] ? base[((size_t)b * B.m + k) * nt + t] : 0.0;
        double x[EM_MAXM], p[EM_MAXM];
#pragma unroll
        for (int k = 0; k < EM_MAXM; ++k) {
            x[k] = 0.0;
            p[k] = 0.0;
        }
#pragma unroll
        for (int c = 0; c < 3 * EM_MAXM; ++c)
#pragma unroll
            for (int k = 0; k < EM_MAXM; ++k) {
                x[k] = x[k] + C[c * EM_MAXM + k] * s[c];
                if (c >= EM_MAXM) p[k] = p[k] + C[(3 * EM_MAXM + c) * EM_MAXM + k] * s[c];
            }
#pragma unroll
        for (int k = 0; k < EM_MAXM; ++k) {
            if (k < B.m) base[(size_t)k * nt + t] = x[k];
            if (k < B.na) base[((size_t)2 * B.m + k) * nt + t] = p[k];
        }
    }
}

__device__ __forceinline__ double em_round(double v, int f32) { return f32 ? (double)(float)v : v; }

// ---- the host's small dense problems
// cyclic Jacobi on a symmetric n×n matrix (row-major, destroyed): eigenvalues ascending in w, the eigenvectors the columns of V
static void em_jacobi(int n, std::vector<double>& A, std::vector<double>& V, std::vector<double>& w) {
    V.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int p = 0; p < n; ++p) {
            dia += A[(size_t)p * n + p] * A[(size_t)p * n + p];
            for (int q = p + 1; q < n; ++q) off += A[(size_t)p * n + q] * A[(size_t)p * n + q];
        }
        if (!(off > 1e-34 * dia)) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[(size_t)q * n + q] - A[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {       // columns p, q
                    const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                    A[(size_t)k * n + p] = c * akp - s * akq;
                    A[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {       // rows p, q
                    const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
                    A[(size_t)p * n + k] = c * apk - s * aqk;
                    A[(size_t)q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
                    V[(size_t)k * n + p] = c * vkp - s * vkq;
                    V[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    std::vector<int> ord(n);
    for (int i = 0; i < n; ++i) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return A[(size_t)a * n + a] < A[(size_t)b * n + b]; });
    std::vector<double> Vs((size_t)n * n);
    w.resize(n);
    for (int j = 0; j < n; ++j) {
        w[j] = A[(size_t)ord[j] * n + ord[j]];
        for (int k = 0; k < n; ++k) Vs[(size_t)k * n + j] = V[(size_t)k * n + ord[j]];
    }
    V.swap(Vs);
}

// Rayleigh–Ritz on the pencil (GA, GM), q×q row-major with the upper triangles valid: C (q×m, row-major) and the m smallest Ritz values.
// 0: done; 1: a Gram matrix is not positive (or fewer than m directions are left); 2: a non-finite entry
static int em_rayleigh_ritz(int q, int m, std::vector<double>& GA, std::vector<double>& GM, std::vector<double>& C, double* theta, int& dropped) {
    for (int i = 0; i < q; ++i)
        for (int j = i; j < q; ++j) {
            if (!std::isfinite(GA[(size_t)i * q + j]) || !std::isfinite(GM[(size_t)i * q + j])) return 2;
            GA[(size_t)j * q + i] = GA[(size_t)i * q + j];
            GM[(size_t)j * q + i] = GM[(size_t)i * q + j];
        }
    std::vector<double> s(q);
    for (int i = 0; i < q; ++i) {
        if (!(GM[(size_t)i * q + i] > 0.0)) return 1;
        s[i] = 1.0 / std::sqrt(GM[(size_t)i * q + i]);
    }
    std::vector<double> Ms((size_t)q * q), As((size_t)q * q), V, mu;
    for (int i = 0; i < q; ++i)
        for (int j = 0; j < q; ++j) {
            Ms[(size_t)i * q + j] = s[i] * GM[(size_t)i * q + j] * s[j];
            As[(size_t)i * q + j] = s[i] * GA[(size_t)i * q + j] * s[j];
        }
    em_jacobi(q, Ms, V, mu);
    const double top = mu[q - 1];
    if (!(top > 0.0)) return 1;
    int first = 0;
    while (first < q && !(mu[first] > 1e-12 * top)) ++first;
    const int r = q - first;
    dropped += first;
    if (r < m) return 1;
    std::vector<double> Bm((size_t)q * r);      // B = V_keep·μ^−½
    for (int k = 0; k < q; ++k)
        for (int j = 0; j < r; ++j) Bm[(size_t)k * r + j] = V[(size_t)k * q + first + j] / std::sqrt(mu[first + j]);
    std::vector<double> AB((size_t)q * r, 0.0), Ar((size_t)r * r, 0.0), Z, th;
    for (int i = 0; i < q; ++i)
        for (int j = 0; j < r; ++j) {
            double a = 0.0;
            for (int k = 0; k < q; ++k) a += As[(size_t)i * q + k] * Bm[(size_t)k * r + j];
            AB[(size_t)i * r + j] = a;
        }
    for (int i = 0; i < r; ++i)
        for (int j = i; j < r; ++j) {
            double a = 0.0;
            for (int k = 0; k < q; ++k) a += Bm[(size_t)k * r + i] * AB[(size_t)k * r + j];
            Ar[(size_t)i * r + j] = Ar[(size_t)j * r + i] = a;
        }
    em_jacobi(r, Ar, Z, th);
    if (!(th[0] > 0.0)) return 1;
    C.assign((size_t)q * m, 0.0);
    for (int i = 0; i < q; ++i)
        for (int k = 0; k < m; ++k) {
            double a = 0.0;
            for (int j = 0; j < r; ++j) a += Bm[(size_t)i * r + j] * Z[(size_t)j * r + k];
            C[(size_t)i * m + k] = s[i] * a;
        }
    for (int k = 0; k < m; ++k) theta[k] = th[k];
    return 0;
}

struct ModesObject {
    int m = 0, solved = 0;
    long long nt = 0;
    double lam[EM_MAXM] = {};
    double *rho = nullptr, *Mn = nullptr, *gout = nullptr, *cdev = nullptr;
    EmBlocks B;
    DevBuf<double> buf, partial;
    DevBuf<unsigned> tickets;
    DevBuf<unsigned long long> cnt;
    PinnedBuf<double> h_out, h_c;
};

// the Gram pass over S = [X, W (na), P (np)] and the Rayleigh–Ritz step: the coefficient matrices go to the device, λ to o.lam
template <class Level>
static int em_gram_rr(LsmHandle* h, MgSolver<Level>& eo, ModesObject& o, int na, int np, const int* act, hipStream_t st, int& dropped, int& rr) {
    const int m = o.m, q = m + na + np, nbq = (q + EM_TILE - 1) / EM_TILE;
    EmTiles tiles;
    memset(&tiles, 0, sizeof(tiles));
    int T = 0;
    for (int bi = 0; bi < nbq; ++bi)
        for (int bj = bi; bj < nbq; ++bj, ++T) {
            tiles.bi[T] = (unsigned char)bi;
            tiles.bj[T] = (unsigned char)bj;
        }
    EmBlocks B = o.B;
    B.na = na; B.np = np;
    const unsigned nb = std::min<unsigned>(mg_blocks(o.nt), EM_GRAMB);
    hipLaunchKernelGGL(em_gram_kernel, dim3(nb, T), dim3(MG_THREADS), 0, st, B, eo.lev[0].nn, tiles, (const double*)o.Mn, o.partial.p, o.tickets.p, o.gout + EM_OUT_GRAM);
    LSM_HIP(h, hipGetLastError());
    LSM_HIP(h, hipMemcpyAsync(o.h_out.p, o.gout, (size_t)T * 32 * sizeof(double), hipMemcpyDeviceToHost, st));
    LSM_HIP(h, hipMemcpyAsync(eo.h_st, eo.st, sizeof(MgState), hipMemcpyDeviceToHost, st));
    LSM_HIP(h, hipStreamSynchronize(st));
    std::vector<double> GA((size_t)q * q, 0.0), GM((size_t)q * q, 0.0), C;
    for (int t = 0; t < T; ++t)
        for (int a = 0; a < EM_TILE; ++a)
            for (int b = 0; b < EM_TILE; ++b) {
                const int i = EM_TILE * tiles.bi[t] + a, j = EM_TILE * tiles.bj[t] + b;
                if (i >= q || j >= q || j < i) continue;
                GA[(size_t)i * q + j] = o.h_out.p[t * 32 + a * EM_TILE + b];
                GM[(size_t)i * q + j] = o.h_out.p[t * 32 + 16 + a * EM_TILE + b];
            }
    double theta[EM_MAXM];
    rr = eo.h_st.p->status != MG_RUN ? 1 : em_rayleigh_ritz(q, m, GA, GM, C, theta, dropped);
    if (rr) return LSM_OK;
    for (int k = 0; k < m; ++k) o.lam[k] = theta[k];
    // the rows in slot order: column c of S sits in slot (block, k)
    double* hc = o.h_c.p;
    memset(hc, 0, 6 * EM_MAXM * EM_MAXM * sizeof(double));
    for (int c = 0; c < q; ++c) {
        const int b = c < m ? 0 : c < m + na ? 1 : 2, k = c - (b == 0 ? 0 : b == 1 ? m : m + na);
        const int row = b * EM_MAXM + k;
        for (int j = 0; j < m; ++j) hc[row * EM_MAXM + j] = C[(size_t)c * m + j];
        if (b > 0)
            for (int j = 0; j < na; ++j) hc[(3 * EM_MAXM + row) * EM_MAXM + j] = C[(size_t)c * m + act[j]];
    }
    LSM_HIP(h, hipMemcpyAsync(o.cdev, hc, 6 * EM_MAXM * EM_MAXM * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(em_update_kernel, dim3(mg_blocks(o.nt), 2), dim3(MG_THREADS), 0, st, B, (const double*)o.cdev);
    LSM_HIP(h, hipGetLastError());
    return LSM_OK;
}

// the solve of lsm_*_modes_solve (fn: the caller's name, for the messages).  apply(na, x, y, stream) enqueues y_j = A x_j for the na
// columns of nt doubles at x, the rows of fixed components zero; the columns hold zero on the fixed components
template <class Level, class Apply>
static int em_solve(LsmHandle* h, MgSolver<Level>& eo, ModesObject& o, const char* fn, Apply apply, const double* x0, double rtol, int max_iters, double* lambda,
                    double* relres, int* iters, int64_t stats[4]) {
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (!(rtol > 0) || !std::isfinite(rtol) || max_iters < 1)
        return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": rtol must be positive and finite and max_iters at least 1");
    const int N = Level::comps(eo.N), m = o.m, nt = (int)o.nt;
    const Level& L = eo.lev[0];
    const int jac = eo.precond == LSM_PRECOND_JACOBI;
    (void)hipSetDevice(h->device);
    hipStream_t st = h->stream;
    const unsigned nbt = mg_blocks(o.nt);
    double* const X = o.B.base;
    double* const W = X + (size_t)m * nt;
    double* const AX = X + (size_t)3 * m * nt;
    double* const AW = X + (size_t)4 * m * nt;
    o.solved = 0;
    LSM_HIP(h, hipMemsetAsync(eo.st, 0, sizeof(MgState), st));     // status MG_RUN: the V-cycle's kernels run
    hipLaunchKernelGGL(em_init_kernel<Level>, dim3(mg_blocks((long long)m * nt)), dim3(MG_THREADS), 0, st, L, N, (long long)m * nt, x0, X);
    apply(m, (const double*)X, AX, st);
    LSM_HIP(h, hipGetLastError());
    int dropped = 0, rr = 0, it = 0, na = 0, np = 0, act[EM_MAXM], why = 0;
    long long applies = 0;
    double rel[EM_MAXM];
    for (int k = 0; k < m; ++k) rel[k] = INFINITY;
    const int r0 = em_gram_rr(h, eo, o, 0, 0, act, st, dropped, rr);
    if (r0 != LSM_OK) return r0;
    if (rr == 2) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + (x0 ? ": x0 must be finite" : ": a non-finite Gram matrix at the start"));
    if (rr) why = 2;
    while (!why) {
        EmLam lam;
        for (int k = 0; k < EM_MAXM; ++k) lam.v[k] = o.lam[k];
        hipLaunchKernelGGL(em_resid_kernel, dim3(nbt), dim3(MG_THREADS), 0, st, o.B, L.nn, lam, (const double*)o.Mn, o.partial.p, o.tickets.p + 31, o.gout + EM_OUT_NORM);
        LSM_HIP(h, hipGetLastError());
        LSM_HIP(h, hipMemcpyAsync(o.h_out.p + EM_OUT_NORM, o.gout + EM_OUT_NORM, 2 * EM_MAXM * sizeof(double), hipMemcpyDeviceToHost, st));
        LSM_HIP(h, hipStreamSynchronize(st));
        na = 0;
        for (int k = 0; k < m; ++k) {
            const double rn = std::sqrt(o.h_out.p[EM_OUT_NORM + 2 * k]), mn = std::sqrt(o.h_out.p[EM_OUT_NORM + 2 * k + 1]);
            rel[k] = rn / (o.lam[k] * mn);
            if (!(rn <= rtol * o.lam[k] * mn)) act[na++] = k;
        }
        if (na == 0) break;
        if (it >= max_iters) { why = 1; break; }
        for (int j = 0; j < na; ++j) {       // W_j = T(R_{act[j]}): ascending, and j ≤ act[j], so no residual is overwritten before its turn
            double* src = W + (size_t)act[j] * nt;
            double* dst = W + (size_t)j * nt;
            if (jac) hipLaunchKernelGGL(em_precond_kernel<Level>, dim3(nbt), dim3(MG_THREADS), 0, st, L, nt, (const double*)src, L.D, dst);
            else {
                mg_vcycle(eo, src, st);
                hipLaunchKernelGGL(em_precond_kernel<Level>, dim3(nbt), dim3(MG_THREADS), 0, st, L, nt, (const double*)eo.xb[0], (const double*)nullptr, dst);
            }
        }
        applies += na;
        apply(na, (const double*)W, AW, st);
        LSM_HIP(h, hipGetLastError());
        const int r1 = em_gram_rr(h, eo, o, na, np, act, st, dropped, rr);
        if (r1 != LSM_OK) return r1;
        if (rr) { why = 2; break; }
        np = na;
        ++it;
    }
    LSM_HIP(h, hipStreamSynchronize(st));
    for (int k = 0; k < m; ++k) {
        if (lambda) lambda[k] = o.lam[k];
        if (relres) relres[k] = rel[k];
    }
    if (iters) *iters = it;
    if (stats) { stats[0] = it; stats[1] = applies; stats[2] = dropped; stats[3] = na; }
    o.solved = 1;
    if (why) {
        char msg[320];
        double worst = 0.0;
        for (int k = 0; k < m; ++k) worst = std::max(worst, rel[k]);
        snprintf(msg, sizeof(msg), "%s: %s: %d iterations, largest relative residual %.3e (rtol %.3e); X is the last iterate", fn,
                 why == 1 ? "no convergence within max_iters" : "a Gram matrix or the preconditioner is not positive", it, worst, rtol);
        return lsm_fail(h, LSM_ERR_NOT_CONVERGED, msg);
    }
    return LSM_OK;
}

// the workspace of lsm_*_modes_create (fn: the caller's name): the blocks, the cell densities from ϕ or the caller's, checked, and the
// node mass.  The caller has checked its arguments
template <class Level>
static int em_create(LsmHandle* h, MgSolver<Level>& eo, ModesObject& o, const char* fn, const void* phi, double level, double rho_in, double rho_out,
                     const double* rho_cells, int m) {
    const int N = eo.N;
    const Level& L = eo.lev[0];
    o.m = m;
    o.nt = (long long)Level::comps(N) * L.nn;
    size_t ncell = 1;
    double hmin = INFINITY;
    for (int d = 0; d < N; ++d) {
        ncell *= (size_t)(L.n[d] - 1);
        hmin = std::min(hmin, L.h[d]);
    }
    const size_t nblk = (size_t)6 * m * (size_t)o.nt;
    LSM_HIP(h, o.buf.alloc((nblk + (size_t)L.nn + ncell + EM_OUT_N + 6 * EM_MAXM * EM_MAXM) * sizeof(double)));
    LSM_HIP(h, o.partial.alloc((size_t)std::max(32 * EM_GRAMB * EM_MAXT, 2 * EM_MAXM * MG_MAXB) * sizeof(double)));
    LSM_HIP(h, o.tickets.alloc(32 * sizeof(unsigned)));
    LSM_HIP(h, o.cnt.alloc(2 * sizeof(unsigned long long)));
    LSM_HIP(h, o.h_out.alloc(EM_OUT_N * sizeof(double)));
    LSM_HIP(h, o.h_c.alloc(6 * EM_MAXM * EM_MAXM * sizeof(double)));
    o.B = EmBlocks{o.buf.p, o.nt, m, 0, 0};
    o.Mn = o.buf.p + nblk;
    o.rho = o.Mn + L.nn;
    o.gout = o.rho + ncell;
    o.cdev = o.gout + EM_OUT_N;
    hipStream_t st = h->stream;
    LSM_HIP(h, hipMemsetAsync(o.tickets.p, 0, 32 * sizeof(unsigned), st));
    LSM_HIP(h, hipMemsetAsync(o.cnt.p, 0, 2 * sizeof(unsigned long long), st));
    MG_LAUNCH2(N, em_rho_kernel, Level, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, eo.F, rho_cells ? (const void*)nullptr : phi, level, rho_in, rho_out, hmin, rho_cells,
               o.rho, o.cnt.p);
    MG_LAUNCH2(N, em_mass_kernel, Level, dim3(mg_blocks(L.nn)), MG_THREADS, st, L, (const double*)o.rho, o.Mn);
    LSM_HIP(h, hipGetLastError());
    unsigned long long c[2] = {0, 0};
    LSM_HIP(h, hipMemcpyAsync(c, o.cnt.p, sizeof(c), hipMemcpyDeviceToHost, st));
    LSM_HIP(h, hipStreamSynchronize(st));
    if (c[0]) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": phi must be finite");
    if (c[1]) return lsm_fail(h, LSM_ERR_INVALID, std::string(fn) + ": the cell densities must be finite and positive");
    return LSM_OK;
}

// (∏h)^−½: a stored mode is X_k times this, so that ∏h·Σ M u² = 1
template <class Level>
static double em_scale(const Level& L, int N) {
    double vol = 1.0;
    for (int d = 0; d < N; ++d) vol = vol * L.h[d];
    return 1.0 / std::sqrt(vol);
}

}  // namespace lsm
