// lsm_quad.hip — quadrature(ϕ; interpolation_order, quadrature_order, surface) on the device: nodes and weights that
// integrate over {ψ < 0} or {ψ = 0} of the piecewise Bernstein interpolant ψ (src/LevelSetMethods.jl:103-126,
// ext/ImplicitIntegrationExt.jl), by R. Saye's algorithm (SIAM J. Sci. Comput. 37(2), 2015) on each cell's patch through
// the four operations the reference's extension supplies: bound (coefficient extrema), gradient (coefficient
// differences), project (face restriction) and split (de Casteljau halving).  tests/_quad_ref.py restates it; the rules:
//   * a box drops every polynomial whose bound excludes 0; with none left it gets the tensor rule (base levels, or a volume box
//     whose top-level polynomial is negative) or nothing;
//   * height direction k = the first arg-max of |∂ψ/∂x_k| at the box centre (ψ: the first polynomial left); every polynomial
//     must be monotone along k, else the box is halved along its first longest side, at most QUAD_DEPTH times per level; a box
//     at the limit gets the fallback (counted): volume, the tensor rule masked by ψ < 0; surface, one node per base node of the
//     tensor rule at the root of its line; base levels, the tensor rule;
//   * the base: lower and upper k-faces of every polynomial, one dimension down, no sign condition; 1-D: roots isolated by
//     Bernstein subdivision (QUAD_ISO halvings at most);
//   * every line through a base node: one root per polynomial (safeguarded Newton–bisection in Bernstein form), the q-point
//     Gauss–Legendre rule on the pieces (volume: where ψ < 0 at the midpoint), or the root with weight w·|∇ψ|/|∂ψ/∂x_k|.
// Every device function is inlined into its kernel: an out-of-line call into the code that runs the wave's barriers on the
// kernel's LDS (the compiler outlined qd_run_level at k = 4, 5 in 3-D) left the 3-D kernels of those orders hanging.
// Kernels: a classify sweep (one thread per cell: empty / cut / full from the coefficient extrema, counts per chunk of cells),
// an ordered compaction of the cut and full lists (ascending linear cell index), and one wavefront per cut cell, run twice
// (count, then emit at the scanned offsets).  A cell's polynomials and their boxes live in LDS (a stack of boxes per level);
// the control flow is uniform over the wave (every lane reads the same LDS values), lane 0 isolates the 1-D roots, and the base
// nodes of the 1-D level are spread over the lanes, each lane lifting its node through the lines of the higher levels.
// fp64 throughout (f32 storage is read as f32 and evaluated in f64).  Compiled as part of lsm_reinit.hip (its patch set-up).

constexpr int QUAD_QMAX = 20;     // Gauss–Legendre points per direction
constexpr int QUAD_DEPTH = 6;     // halvings of a box per level
constexpr int QUAD_ISO = 16;      // halvings of an interval while isolating 1-D roots
constexpr int QUAD_ITERS = 64;    // Newton–bisection steps
constexpr int QUAD_CHUNK = 4096;  // cells per workgroup of the classify and compaction kernels
constexpr double QUAD_EPS = 2.220446049250313e-16;
enum { QUAD_NONE = 0, QUAD_VOL = 1, QUAD_SURF = 2 };
enum { QK_EMPTY = 0, QK_MONO = 1, QK_TENSOR = 2, QK_FB_VOL = 3, QK_FB_SURF = 4 };

struct QuadArgs {
    ReinitArgs a;
    int q, surface;
    double gx[QUAD_QMAX], gw[QUAD_QMAX];   // Gauss–Legendre nodes (ascending) and weights on [0, 1]
};

constexpr int qpow(int b, int e) { return e == 0 ? 1 : b * qpow(b, e - 1); }
// polynomials left in a box are a bit mask (a small array indexed at run time would live in scratch memory)
__device__ __forceinline__ int qd_nth(unsigned m, int a) {
    for (int i = 0; i < a; ++i) m &= m - 1;
    return __ffs(m) - 1;
}
__device__ __forceinline__ int qd_stride(int d, int nc) { return d == 0 ? 1 : (d == 1 ? nc : nc * nc); }

// ---- 1-D Bernstein polynomials in registers
template <int NC>
__device__ __forceinline__ void qd_decas(const double* bin, double t, double& f, double& df) {
    double b[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) b[i] = bin[i];
    const double s = 1.0 - t;
#pragma unroll
    for (int r = NC - 1; r > 1; --r)
#pragma unroll
        for (int i = 0; i < r; ++i) b[i] = s * b[i] + t * b[i + 1];
    f = s * b[0] + t * b[1];
    df = (double)(NC - 1) * (b[1] - b[0]);
}
template <int NC>
__device__ __forceinline__ double qd_val(const double* b, double t) { double f, df; qd_decas<NC>(b, t, f, df); return f; }

// the crossing of sign(v < 0) on [0, 1] (b[0] and b[NC-1] differ in it): safeguarded Newton–bisection
template <int NC>
__device__ __forceinline__ double qd_root(const double* b) {
    const bool s0 = b[0] < 0.0;
    double lo = 0.0, hi = 1.0, t = 0.5;
    for (int it = 0; it < QUAD_ITERS; ++it) {
        double f, df;
        qd_decas<NC>(b, t, f, df);
        if (f == 0.0) return t;
        if ((f < 0.0) == s0) lo = t; else hi = t;
        double tn = df != 0.0 ? t - f / df : -1.0;
        if (!(lo < tn && tn < hi)) tn = 0.5 * (lo + hi);
        if (fabs(tn - t) <= 4.0 * QUAD_EPS) return tn;
        t = tn;
    }
    return t;
}

// the 1-D polynomial along axis `keep` of an L-dimensional coefficient array (axis 0 fastest) at the local parameters ts of the
// other axes, the highest axis contracted first
template <int L, int NC>
__device__ __forceinline__ void qd_contract(const double* c, int keep, const double ts[3], double out[NC]) {
    if constexpr (L == 1) {
#pragma unroll
        for (int i = 0; i < NC; ++i) out[i] = c[i];
    } else if constexpr (L == 2) {
        const int o = 1 - keep, sk = keep ? NC : 1, so = o ? NC : 1;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            double f[NC];
#pragma unroll
            for (int m = 0; m < NC; ++m) f[m] = c[i * sk + m * so];
            out[i] = qd_val<NC>(f, ts[o]);
        }
    } else {
        const int a = keep == 0 ? 1 : 0, b = keep == 2 ? 1 : 2;
        const int sk = qd_stride(keep, NC), sa = qd_stride(a, NC), sb = qd_stride(b, NC);
        // one fiber at a time (not unrolled: unrolled, the NC³ loads are hoisted together and the 3-D cell kernels spill)
#pragma unroll 1
        for (int i = 0; i < NC; ++i) {
            double r[NC];
#pragma unroll 1
            for (int ia = 0; ia < NC; ++ia) {
                double f[NC];
#pragma unroll
                for (int m = 0; m < NC; ++m) f[m] = c[i * sk + ia * sa + m * sb];
                const double v = qd_val<NC>(f, ts[b]);
#pragma unroll
                for (int j = 0; j < NC; ++j)
                    if (j == ia) r[j] = v;
            }
            const double v = qd_val<NC>(r, ts[a]);
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (j == i) out[j] = v;
        }
    }
}

// ---- the LDS of one wavefront
template <int L, int NP, int NC>
struct QLevel {                 // a stack of L-dimensional boxes with up to NP polynomials each
    static constexpr int NCL = qpow(NC, L);
    double c[QUAD_DEPTH + 1][NP][NCL];
    double lo[QUAD_DEPTH + 1][L], hi[QUAD_DEPTH + 1][L];
    int np[QUAD_DEPTH + 1], depth[QUAD_DEPTH + 1];
    int sp, kind, k, nalive;
    unsigned alive;             // the polynomials left in the box being processed (bit mask)
};
template <int NP, int NC>
struct QLine {                  // the 1-D level: polynomials, root isolation (lane 0), and its nodes
    static constexpr int MAXR = NP * (NC - 1);
    double c[NP][NC];
    double lo, hi;
    int np;
    double stk[QUAD_ISO + 2][NC], st0[QUAD_ISO + 2], st1[QUAD_ISO + 2];
    int sd[QUAD_ISO + 2];
    double roots[MAXR];
    int n1;
    double x1[(MAXR + 1) * QUAD_QMAX], w1[(MAXR + 1) * QUAD_QMAX];
};
template <int N, int NC> struct QuadShared;
template <int NC> struct QuadShared<1, NC> {
    QLine<1, NC> l1;
    double tA[qpow(NC + 1, 1)], tB[qpow(NC + 1, 1)];
};
template <int NC> struct QuadShared<2, NC> {
    QLevel<2, 1, NC> l2;
    QLine<2, NC> l1;
    double tA[qpow(NC + 1, 2)], tB[qpow(NC + 1, 2)];
};
template <int NC> struct QuadShared<3, NC> {
    QLevel<3, 1, NC> l3;
    QLevel<2, 2, NC> l2;
    QLine<4, NC> l1;
    double tA[qpow(NC + 1, 3)], tB[qpow(NC + 1, 3)];
};
template <int L, int N, int NC>
__device__ __forceinline__ auto& qlev(QuadShared<N, NC>& S) {
    if constexpr (N == 3 && L == 3) return S.l3;
    else return S.l2;
}

// where a lane's nodes go: counted, or written at base + cnt (never beyond the count of the count pass)
struct QuadSink {
    int cnt;
    bool write;
    long long base;
    int limit;
    double* coords;
    double* weights;
};
template <int N>
__device__ __forceinline__ void qd_put(QuadSink& o, const double x[3], double w) {
    if (o.write && o.cnt < o.limit) {
        const long long p = o.base + o.cnt;
#pragma unroll
        for (int d = 0; d < N; ++d) o.coords[p * N + d] = x[d];
        o.weights[p] = w;
    }
    ++o.cnt;
}

// gradient of an L-dimensional polynomial at local parameters ts (physical units)
template <int L, int NC>
__device__ __forceinline__ void qd_grad(const double* c, const double ts[3], const double* lo, const double* hi, double g[3]) {
#pragma unroll
    for (int j = 0; j < L; ++j) {
        double line[NC], f, df;
        qd_contract<L, NC>(c, j, ts, line);
        qd_decas<NC>(line, ts[j], f, df);
        g[j] = df / (hi[j] - lo[j]);
    }
}

template <int L, int N, int NC>
__device__ __forceinline__ void qd_lift(const QuadArgs& qa, QuadShared<N, NC>& S, const double* y, double wy, int topmode, QuadSink& o);

// the node x (L coordinates) with weight w of level L: final (L == N) or a base node of level L + 1
template <int L, int N, int NC>
__device__ __forceinline__ void qd_next(const QuadArgs& qa, QuadShared<N, NC>& S, const double* x, double w, int topmode, QuadSink& o) {
    if constexpr (L == N) qd_put<N>(o, x, w);
    else qd_lift<L + 1, N, NC>(qa, S, x, w, topmode, o);
}

// surface node on the line of level L through base point y at root r of ψ's line b
template <int L, int N, int NC>
__device__ __forceinline__ void qd_surface_node(const QuadArgs& qa, QuadShared<N, NC>& S, const double* c, const double* b, double r, const double* y,
                                                double wy, int k, const double* lo, const double* hi, int topmode, QuadSink& o) {
    double ts[3] = {0.0, 0.0, 0.0}, x[3] = {0.0, 0.0, 0.0};
    for (int j = 0, m = 0; j < L; ++j) {
        if (j == k) continue;
        ts[j] = (y[m] - lo[j]) / (hi[j] - lo[j]);
        x[j] = y[m];
        ++m;
    }
    ts[k] = r;
    double g[3];
    qd_grad<L, NC>(c, ts, lo, hi, g);
    double f, df;
    qd_decas<NC>(b, r, f, df);
    g[k] = df / (hi[k] - lo[k]);
    double acc = 0.0;
    for (int j = 0; j < L; ++j) acc += g[j] * g[j];
    x[k] = lo[k] + r * (hi[k] - lo[k]);
    qd_next<L, N, NC>(qa, S, x, wy * (sqrt(acc) / fabs(g[k])), topmode, o);
}

// Gauss–Legendre nodes on the pieces [u, v] of a line of level L (roots sorted); psi: only where psi(midpoint) < 0
template <int L, int N, int NC>
__device__ __forceinline__ void qd_pieces(const QuadArgs& qa, QuadShared<N, NC>& S, double r0, double r1, int nr, const double* y, double wy, int k,
                                          const double* lo, const double* hi, const double* psi, int topmode, QuadSink& o) {
    const double hk = hi[k] - lo[k];
    double x[3] = {0.0, 0.0, 0.0};
    for (int j = 0, m = 0; j < L; ++j)
        if (j != k) x[j] = y[m++];
    for (int p = 0; p <= nr; ++p) {
        const double u = p == 0 ? 0.0 : (p == 1 ? r0 : r1), v = p == nr ? 1.0 : (p == 0 ? r0 : r1);
        if (!(v > u)) continue;
        if (psi && !(qd_val<NC>(psi, 0.5 * (u + v)) < 0.0)) continue;
        for (int i = 0; i < qa.q; ++i) {
            x[k] = lo[k] + (u + (v - u) * qa.gx[i]) * hk;
            qd_next<L, N, NC>(qa, S, x, wy * ((v - u) * qa.gw[i] * hk), topmode, o);
        }
    }
}

// one base node y (L-1 coordinates, weight wy) of the current box of level L >= 2: the line along k through it
template <int L, int N, int NC>
__device__ __forceinline__ void qd_lift(const QuadArgs& qa, QuadShared<N, NC>& S, const double* y, double wy, int topmode, QuadSink& o) {
    auto& lv = qlev<L, N, NC>(S);
    const int s = lv.sp - 1, k = lv.k, kind = lv.kind;
    const unsigned alive = lv.alive;
    const double* lo = lv.lo[s];
    const double* hi = lv.hi[s];
    const int mode = L == N ? topmode : QUAD_NONE;
    double ts[3] = {0.0, 0.0, 0.0};
    for (int j = 0, m = 0; j < L; ++j) {
        if (j == k) continue;
        ts[j] = (y[m] - lo[j]) / (hi[j] - lo[j]);
        ++m;
    }
    if (kind == QK_TENSOR) {
        qd_pieces<L, N, NC>(qa, S, 0.0, 0.0, 0, y, wy, k, lo, hi, nullptr, topmode, o);
        return;
    }
    if (kind == QK_FB_VOL) {                  // the tensor rule along the last axis, kept where ψ < 0
        double b[NC];
        qd_contract<L, NC>(lv.c[s][qd_nth(alive, 0)], k, ts, b);
        const double hk = hi[k] - lo[k];
        double x[3] = {0.0, 0.0, 0.0};
        for (int j = 0, m = 0; j < L; ++j)
            if (j != k) x[j] = y[m++];
        for (int i = 0; i < qa.q; ++i) {
            x[k] = lo[k] + (0.0 + (1.0 - 0.0) * qa.gx[i]) * hk;
            if (qd_val<NC>(b, qa.gx[i]) < 0.0) qd_next<L, N, NC>(qa, S, x, wy * ((1.0 - 0.0) * qa.gw[i] * hk), topmode, o);
        }
        return;
    }
    if (kind == QK_FB_SURF) {
        double b[NC];
        const double* c = lv.c[s][qd_nth(alive, 0)];
        qd_contract<L, NC>(c, k, ts, b);
        if ((b[0] < 0.0) != (b[NC - 1] < 0.0)) qd_surface_node<L, N, NC>(qa, S, c, b, qd_root<NC>(b), y, wy, k, lo, hi, topmode, o);
        return;
    }
    // QK_MONO: one root per polynomial at most (a box holds at most two polynomials from level 2 up)
    double r0 = 0.0, r1 = 0.0;
    int nr = 0;
    double b0[NC];
    for (int a = 0; a < lv.nalive; ++a) {
        double b[NC];
        qd_contract<L, NC>(lv.c[s][qd_nth(alive, a)], k, ts, b);
        if (a == 0)
#pragma unroll
            for (int i = 0; i < NC; ++i) b0[i] = b[i];
        if ((b[0] < 0.0) != (b[NC - 1] < 0.0)) {
            const double r = qd_root<NC>(b);
            if (nr == 0) r0 = r;
            else if (r < r0) { r1 = r0; r0 = r; }
            else r1 = r;
            ++nr;
        }
    }
    if (mode == QUAD_SURF) {
        if (nr) qd_surface_node<L, N, NC>(qa, S, lv.c[s][qd_nth(alive, 0)], b0, r0, y, wy, k, lo, hi, topmode, o);
        return;
    }
    qd_pieces<L, N, NC>(qa, S, r0, r1, nr, y, wy, k, lo, hi, mode == QUAD_VOL ? b0 : nullptr, topmode, o);
}

// ---- the 1-D level (lane 0): roots of every polynomial by subdivision, then its nodes into LDS
template <int NP, int NC>
__device__ __forceinline__ void qd_line1(const QuadArgs& qa, QLine<NP, NC>& l, int mode) {
    l.n1 = 0;
    unsigned alive = 0;
    int na = 0;
    for (int a = 0; a < l.np; ++a) {
        double m = l.c[a][0], M = l.c[a][0];
        for (int i = 1; i < NC; ++i) { m = fmin(m, l.c[a][i]); M = fmax(M, l.c[a][i]); }
        if (!(m > 0.0 || M < 0.0)) { alive |= 1u << a; ++na; }
    }
    const double hk = l.hi - l.lo;
    auto piece_nodes = [&](double u, double v) {
        for (int i = 0; i < qa.q; ++i) {
            l.x1[l.n1] = l.lo + (u + (v - u) * qa.gx[i]) * hk;
            l.w1[l.n1] = 1.0 * ((v - u) * qa.gw[i] * hk);
            ++l.n1;
        }
    };
    if (na == 0) {
        bool neg = false;
        if (mode == QUAD_VOL) {
            double M = l.c[0][0];
            for (int i = 1; i < NC; ++i) M = fmax(M, l.c[0][i]);
            neg = M < 0.0;
        }
        if (mode == QUAD_NONE || neg) piece_nodes(0.0, 1.0);
        return;
    }
    int nr = 0;
    for (int a = 0; a < na; ++a) {
        int sp = 0;
        const int pa = qd_nth(alive, a);
        for (int i = 0; i < NC; ++i) l.stk[0][i] = l.c[pa][i];
        l.st0[0] = 0.0; l.st1[0] = 1.0; l.sd[0] = 0; sp = 1;
        while (sp > 0) {
            --sp;
            double b[NC];
            for (int i = 0; i < NC; ++i) b[i] = l.stk[sp][i];
            const double t0 = l.st0[sp], t1 = l.st1[sp];
            const int depth = l.sd[sp];
            int nneg = 0;
            for (int i = 0; i < NC; ++i) nneg += b[i] < 0.0;
            if (nneg == 0 || nneg == NC) continue;
            double dmin = b[1] - b[0], dmax = dmin;
            for (int i = 1; i + 1 < NC; ++i) { const double d = b[i + 1] - b[i]; dmin = fmin(dmin, d); dmax = fmax(dmax, d); }
            if (dmin > 0.0 || dmax < 0.0 || depth == QUAD_ISO) {
                if ((b[0] < 0.0) != (b[NC - 1] < 0.0) && nr < QLine<NP, NC>::MAXR) {
                    const double r = t0 + qd_root<NC>(b) * (t1 - t0);
                    int p = nr++;
                    while (p > 0 && l.roots[p - 1] > r) { l.roots[p] = l.roots[p - 1]; --p; }
                    l.roots[p] = r;
                }
                continue;
            }
            double L[NC], R[NC];
            L[0] = b[0]; R[NC - 1] = b[NC - 1];
            for (int r = NC - 1; r > 0; --r) {
                for (int i = 0; i < r; ++i) b[i] = 0.5 * (b[i] + b[i + 1]);
                L[NC - r] = b[0];
                R[r - 1] = b[r - 1];
            }
            const double tm = 0.5 * (t0 + t1);
            for (int i = 0; i < NC; ++i) { l.stk[sp][i] = R[i]; l.stk[sp + 1][i] = L[i]; }
            l.st0[sp] = tm; l.st1[sp] = t1; l.sd[sp] = depth + 1;
            l.st0[sp + 1] = t0; l.st1[sp + 1] = tm; l.sd[sp + 1] = depth + 1;
            sp += 2;
        }
    }
    if (mode == QUAD_SURF) {
        for (int p = 0; p < nr; ++p) { l.x1[l.n1] = l.lo + l.roots[p] * hk; l.w1[l.n1] = 1.0; ++l.n1; }
        return;
    }
    for (int p = 0; p <= nr; ++p) {
        const double u = p == 0 ? 0.0 : l.roots[p - 1], v = p == nr ? 1.0 : l.roots[p];
        if (!(v > u)) continue;
        if (mode == QUAD_VOL && !(qd_val<NC>(l.c[qd_nth(alive, 0)], 0.5 * (u + v)) < 0.0)) continue;
        piece_nodes(u, v);
    }
}

__device__ __forceinline__ int qd_wave_excl(int v, int& total) {
    const int x = wave_incl_scan(v);
    total = __shfl(x, 63, 64);
    return x - v;
}

// the 1-D level is set up: its nodes, then every node lifted through the lines of the levels above, 64 at a time
template <int N, int NC>
__device__ __forceinline__ void qd_run_line(const QuadArgs& qa, QuadShared<N, NC>& S, int topmode, QuadSink& o, bool emit, int& cursor) {
    const int lane = threadIdx.x;
    if (lane == 0) qd_line1(qa, S.l1, N == 1 ? topmode : QUAD_NONE);
    __syncthreads();
    const int n1 = S.l1.n1;
    for (int b = 0; b < n1; b += 64) {
        const int i = b + lane;
        const double y = i < n1 ? S.l1.x1[i] : 0.0, wy = i < n1 ? S.l1.w1[i] : 0.0;
        // pass 0 counts the lane's nodes; in the emit kernel pass 1 writes them after the wave's scan (one call site: two
        // inlined copies of the lift spill at k = 3 in 3-D)
        int ex = 0, tot = 0;
        for (int pass = 0; pass < (emit ? 2 : 1); ++pass) {
            QuadSink c = o;
            c.cnt = pass ? cursor + ex : 0;
            c.write = pass == 1;
            if (i < n1) {
                if constexpr (N == 1) { const double x[3] = {y, 0.0, 0.0}; qd_put<1>(c, x, wy); }
                else qd_lift<2, N, NC>(qa, S, &y, wy, topmode, c);
            }
            if (pass == 0) {
                if (emit) ex = qd_wave_excl(c.cnt, tot);
                else o.cnt += c.cnt;
            }
        }
        cursor += tot;
    }
    __syncthreads();
}

// the boxes of level L >= 2, depth first; every box that ends as a leaf sets up the level below it and runs it
template <int L, int N, int NC>
__device__ __forceinline__ void qd_run_level(const QuadArgs& qa, QuadShared<N, NC>& S, int topmode, QuadSink& o, bool emit, int& cursor, unsigned* nfb) {
    auto& lv = qlev<L, N, NC>(S);
    constexpr int NCL = qpow(NC, L);
    const int lane = threadIdx.x;
    const int mode = L == N ? topmode : QUAD_NONE;
    while (lv.sp > 0) {
        const int s = lv.sp - 1;
        const int np = lv.np[s];
        unsigned alive = 0;
        int na = 0;
        for (int a = 0; a < np; ++a) {
            double m = lv.c[s][a][0], M = m;
            for (int i = 1; i < NCL; ++i) { m = fmin(m, lv.c[s][a][i]); M = fmax(M, lv.c[s][a][i]); }
            if (!(m > 0.0 || M < 0.0)) { alive |= 1u << a; ++na; }
        }
        int kind = QK_EMPTY, k = L - 1;
        if (na == 0) {
            bool neg = false;
            if (mode == QUAD_VOL) {
                double M = lv.c[s][0][0];
                for (int i = 1; i < NCL; ++i) M = fmax(M, lv.c[s][0][i]);
                neg = M < 0.0;
            }
            kind = mode == QUAD_NONE || neg ? QK_TENSOR : QK_EMPTY;
        } else {
            const double half[3] = {0.5, 0.5, 0.5};
            double g[3];
            qd_grad<L, NC>(lv.c[s][qd_nth(alive, 0)], half, lv.lo[s], lv.hi[s], g);
            k = 0;
            double best = fabs(g[0]);
            for (int j = 1; j < L; ++j)
                if (fabs(g[j]) > best) { k = j; best = fabs(g[j]); }
            bool mono = true;
            for (int a = 0; a < na && mono; ++a) {
                const double* c = lv.c[s][qd_nth(alive, a)];
                const int sk = qd_stride(k, NC);
                double dmin = __builtin_inf(), dmax = -__builtin_inf();
                for (int i = 0; i < NCL; ++i) {
                    if ((i / sk) % NC == NC - 1) continue;
                    const double d = c[i + sk] - c[i];
                    dmin = fmin(dmin, d); dmax = fmax(dmax, d);
                }
                mono = dmin > 0.0 || dmax < 0.0;
            }
            if (mono) {
                kind = QK_MONO;
            } else if (lv.depth[s] == QUAD_DEPTH) {
                if (!emit && lane == 0) atomicAdd(nfb, 1u);
                if (mode == QUAD_VOL) { kind = QK_FB_VOL; k = L - 1; }
                else if (mode == QUAD_SURF) kind = QK_FB_SURF;
                else { kind = QK_TENSOR; k = L - 1; }
            } else {
                // halve along the first longest side: the right half replaces the box, the left half goes on top
                int j = 0;
                double w = lv.hi[s][0] - lv.lo[s][0];
                for (int d = 1; d < L; ++d)
                    if (lv.hi[s][d] - lv.lo[s][d] > w) { j = d; w = lv.hi[s][d] - lv.lo[s][d]; }
                __syncthreads();
                // one fiber per lane (at most 2·6 or 36 fibers): every lane reads its fiber of the box before any lane writes the halves
                constexpr int NF = NCL / NC;
                const int sj = qd_stride(j, NC);
                const bool has = lane < na * NF;
                int a = 0, base = 0;
                double Lc[NC], Rc[NC];
                if (has) {
                    a = lane / NF;
                    for (int d = 0, rr = lane % NF; d < L; ++d) {
                        if (d == j) continue;
                        base += (rr % NC) * qd_stride(d, NC);
                        rr /= NC;
                    }
                    const double* c = lv.c[s][qd_nth(alive, a)];
                    double b[NC];
#pragma unroll
                    for (int i = 0; i < NC; ++i) b[i] = c[base + i * sj];
                    Lc[0] = b[0]; Rc[NC - 1] = b[NC - 1];
#pragma unroll
                    for (int rr = NC - 1; rr > 0; --rr) {
#pragma unroll
                        for (int i = 0; i < rr; ++i) b[i] = 0.5 * (b[i] + b[i + 1]);
                        Lc[NC - rr] = b[0];
                        Rc[rr - 1] = b[rr - 1];
                    }
                }
                __syncthreads();
                if (has) {
#pragma unroll
                    for (int i = 0; i < NC; ++i) { lv.c[s + 1][a][base + i * sj] = Lc[i]; lv.c[s][a][base + i * sj] = Rc[i]; }
                }
                __syncthreads();
                if (lane == 0) {
                    const double mid = lv.lo[s][j] + (lv.hi[s][j] - lv.lo[s][j]) * 0.5;
                    for (int d = 0; d < L; ++d) { lv.lo[s + 1][d] = lv.lo[s][d]; lv.hi[s + 1][d] = lv.hi[s][d]; }
                    lv.hi[s + 1][j] = mid;
                    lv.lo[s][j] = mid;
                    lv.depth[s] = lv.depth[s + 1] = lv.depth[s] + 1;
                    lv.np[s] = lv.np[s + 1] = na;
                    lv.sp = s + 2;
                }
                __syncthreads();
                continue;
            }
        }
        if (kind != QK_EMPTY) {
            __syncthreads();
            if (lane == 0) {
                lv.kind = kind; lv.k = k; lv.nalive = na; lv.alive = alive;
            }
            // the base one level down: the k-faces of the polynomials left (monotone box), none otherwise
            const int nb = kind == QK_MONO ? 2 * na : 0;
            constexpr int NCB = NCL / NC;
            if constexpr (L - 1 == 1) {
                auto& b = S.l1;
                for (int e = lane; e < nb * NCB; e += 64) {
                    const int p = e / NCB, i = e % NCB;
                    const double* c = lv.c[s][qd_nth(alive, p / 2)];
                    b.c[p][i] = c[i * qd_stride(1 - k, NC) + (p % 2 ? (NC - 1) * qd_stride(k, NC) : 0)];
                }
                if (lane == 0) {
                    b.np = nb;
                    b.lo = lv.lo[s][1 - k];
                    b.hi = lv.hi[s][1 - k];
                }
            } else {
                auto& b = qlev<L - 1, N, NC>(S);
                for (int e = lane; e < nb * NCB; e += 64) {
                    const int p = e / NCB, i = e % NCB;
                    const double* c = lv.c[s][qd_nth(alive, p / 2)];
                    // face index i over the axes != k (ascending), at k = 0 or NC - 1
                    int idx = 0;
                    for (int d = 0, rr = i; d < L; ++d) {
                        if (d == k) continue;
                        idx += (rr % NC) * qd_stride(d, NC);
                        rr /= NC;
                    }
                    b.c[0][p][i] = c[idx + (p % 2 ? (NC - 1) * qd_stride(k, NC) : 0)];
                }
                if (lane == 0) {
                    for (int d = 0, m = 0; d < L; ++d) {
                        if (d == k) continue;
                        b.lo[0][m] = lv.lo[s][d];
                        b.hi[0][m] = lv.hi[s][d];
                        ++m;
                    }
                    b.np[0] = nb;
                    b.depth[0] = 0;
                    b.sp = 1;
                }
            }
            __syncthreads();
            if constexpr (L - 1 == 1) qd_run_line<N, NC>(qa, S, topmode, o, emit, cursor);
            else qd_run_level<L - 1, N, NC>(qa, S, topmode, o, emit, cursor, nfb);
        }
        __syncthreads();
        if (lane == 0) lv.sp = s;
        __syncthreads();
    }
}

// ---- kernels
// one cell: its Bernstein coefficients (M along every axis, lanes over the outputs) into the first box of the top level
template <int N, int NC>
__device__ __forceinline__ void qd_cell_coeffs(const QuadArgs& qa, QuadShared<N, NC>& S, const int I[3], double* c) {
    const ReinitArgs& a = qa.a;
    const int nv = a.nv, lane = threadIdx.x;
    const int v1 = N > 1 ? nv : 1, v2 = N > 2 ? nv : 1;
    const long long q0 = a.origin + (I[0] + a.off) + (N > 1 ? (I[1] + a.off) * a.s1 : 0) + (N > 2 ? (I[2] + a.off) * a.s2 : 0);
    for (int e = lane; e < nv * v1 * v2; e += 64) {
        const int j0 = e % nv, j1 = (e / nv) % v1, j2 = e / (nv * v1);
        S.tA[e] = ld_val(a.phi, q0 + j0 + j1 * a.s1 + j2 * a.s2, a.f32);
    }
    __syncthreads();
    double* out0 = N == 1 ? c : S.tB;
    for (int e = lane; e < NC * v1 * v2; e += 64) {          // axis 0: (nv, v1, v2) -> (NC, v1, v2)
        const int i = e % NC, r = e / NC;
        double acc = 0.0;
        for (int j = 0; j < nv; ++j) acc += a.M[i * nv + j] * S.tA[j + nv * r];
        out0[e] = acc;
    }
    __syncthreads();
    if constexpr (N > 1) {
        double* out1 = N == 2 ? c : S.tA;
        for (int e = lane; e < NC * NC * v2; e += 64) {      // axis 1: (NC, v1, v2) -> (NC, NC, v2)
            const int i0 = e % NC, i1 = (e / NC) % NC, j2 = e / (NC * NC);
            double acc = 0.0;
            for (int j = 0; j < nv; ++j) acc += a.M[i1 * nv + j] * S.tB[i0 + NC * (j + v1 * j2)];
            out1[e] = acc;
        }
        __syncthreads();
    }
    if constexpr (N > 2) {
        for (int e = lane; e < NC * NC * NC; e += 64) {      // axis 2
            const int i01 = e % (NC * NC), i2 = e / (NC * NC);
            double acc = 0.0;
            for (int j = 0; j < nv; ++j) acc += a.M[i2 * nv + j] * S.tA[i01 + NC * NC * j];
            c[e] = acc;
        }
        __syncthreads();
    }
}

// counts (EMIT = false) or writes (EMIT = true) the nodes of every candidate cut cell; one wavefront per cell
template <int N, int NC, bool EMIT>
__global__ void __launch_bounds__(64) quad_cells_kernel(QuadArgs qa, const long long* cand, long long ncand, unsigned* counts,
                                                        const long long* node_off, const long long* pos, double* coords, double* weights,
                                                        long long* out_cells, long long* out_offsets, unsigned* nfb) {
    __shared__ QuadShared<N, NC> S;
    const ReinitArgs& a = qa.a;
    const int lane = threadIdx.x;
    const int topmode = qa.surface ? QUAD_SURF : QUAD_VOL;
    for (long long ci = blockIdx.x; ci < ncand; ci += gridDim.x) {
        if (EMIT && counts[ci] == 0) continue;
        const long long cell = cand[ci];
        int I[3];
        cell_unlin(a, cell, I);
        double lo[3], hi[3];
        for (int d = 0; d < N; ++d) { lo[d] = a.lc[d] + (double)(I[d] + a.goff[d]) * a.h[d]; hi[d] = lo[d] + a.h[d]; }
        QuadSink o{0, false, 0, 0, coords, weights};
        if (EMIT) { o.base = node_off[ci]; o.limit = (int)counts[ci]; }
        int cursor = 0;
        if constexpr (N == 1) {
            qd_cell_coeffs<N, NC>(qa, S, I, S.l1.c[0]);
            if (lane == 0) { S.l1.np = 1; S.l1.lo = lo[0]; S.l1.hi = hi[0]; }
            __syncthreads();
            qd_run_line<N, NC>(qa, S, topmode, o, EMIT, cursor);
        } else {
            auto& top = qlev<N, N, NC>(S);
            qd_cell_coeffs<N, NC>(qa, S, I, top.c[0][0]);
            if (lane == 0) {
                for (int d = 0; d < N; ++d) { top.lo[0][d] = lo[d]; top.hi[0][d] = hi[d]; }
                top.np[0] = 1; top.depth[0] = 0; top.sp = 1;
            }
            __syncthreads();
            qd_run_level<N, N, NC>(qa, S, topmode, o, EMIT, cursor, nfb);
        }
        if (!EMIT) {
            const int c = wave_sum(o.cnt);
            if (lane == 0) counts[ci] = (unsigned)c;
        } else if (lane == 0) {
            out_cells[pos[ci]] = cell;
            out_offsets[pos[ci]] = node_off[ci];
        }
        __syncthreads();
    }
}

// classify: 0 empty, 1 cut, 2 full (volume: every coefficient < 0); band fields: cells whose 2^N corners are active only.
// Per chunk of QUAD_CHUNK cells the numbers of cut and full cells.
template <int NV, int NC, int NDIM>   // NV = 0: the general version
__global__ void __launch_bounds__(256) quad_classify_kernel(QuadArgs qa, long long ncell, unsigned char* cls, unsigned* ncut_chunk,
                                                            unsigned* nfull_chunk) {
    const ReinitArgs& a = qa.a;
    __shared__ unsigned wsum[2][4];
    unsigned mc = 0, mf = 0;
    const long long c0 = (long long)blockIdx.x * QUAD_CHUNK;
    for (int r = threadIdx.x; r < QUAD_CHUNK; r += blockDim.x) {
        const long long c = c0 + r;
        if (c >= ncell) break;
        int I[3];
        cell_unlin(a, c, I);
        unsigned char k = 0;
        bool active = true;
        if (a.mask) {
            const long long n0 = a.origin + I[0] + (NDIM > 1 ? I[1] * a.s1 : 0) + (NDIM > 2 ? I[2] * a.s2 : 0);
            for (int e = 0; e < (1 << NDIM); ++e)
                active = active && a.mask[n0 + (e & 1) + (NDIM > 1 && (e & 2) ? a.s1 : 0) + (NDIM > 2 && (e & 4) ? a.s2 : 0)];
        }
        if (active) {
            const long long q0 = a.origin + (I[0] + a.off) + (NDIM > 1 ? (I[1] + a.off) * a.s1 : 0) + (NDIM > 2 ? (I[2] + a.off) * a.s2 : 0);
            double lo, hi;
            if constexpr (NV == 0) bernstein_extrema(a, q0, lo, hi);
            else bernstein_extrema_reg<NV, NC, NDIM>(a, q0, lo, hi);
            if (qa.surface) k = lo * hi > 0.0 ? 0 : 1;          // proven_empty(…; surface = true)
            else k = lo > 0.0 ? 0 : (hi < 0.0 ? 2 : 1);
        }
        cls[c] = k;
        mc += k == 1;
        mf += k == 2;
    }
    mc = block_sum<4>(mc, wsum[0]);
    mf = block_sum<4>(mf, wsum[1]);
    if (threadIdx.x == 0) { ncut_chunk[blockIdx.x] = mc; nfull_chunk[blockIdx.x] = mf; }
}

// the cut and the full cells of every chunk, in ascending order, at the chunk's scanned offsets
__global__ void __launch_bounds__(256) quad_compact_kernel(const unsigned char* cls, long long ncell, const long long* off_cut,
                                                           const long long* off_full, long long* cand, long long* full) {
    constexpr int PER = QUAD_CHUNK / 256;
    __shared__ unsigned wsum[2][4];
    const long long c0 = (long long)blockIdx.x * QUAD_CHUNK + (long long)threadIdx.x * PER;
    unsigned mc = 0, mf = 0;
    for (int e = 0; e < PER; ++e) {
        const long long c = c0 + e;
        const unsigned char k = c < ncell ? cls[c] : 0;
        mc += k == 1; mf += k == 2;
    }
    unsigned total;
    long long pc = off_cut[blockIdx.x] + block_excl_scan<4>(mc, wsum[0], total), pf = off_full[blockIdx.x] + block_excl_scan<4>(mf, wsum[1], total);
    for (int e = 0; e < PER; ++e) {
        const long long c = c0 + e;
        if (c >= ncell) break;
        const unsigned char k = cls[c];
        if (k == 1) cand[pc++] = c;
        else if (k == 2) full[pf++] = c;
    }
}

// sum of n weights in one workgroup, in a fixed order
__global__ void __launch_bounds__(1024) quad_sum_kernel(const double* w, long long n, double* out) {
    __shared__ double s[1024];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) acc += w[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// ---- host side
struct QuadObject {
    DevBuf<long long> cells, offsets, full;
    DevBuf<double> coords, weights, sum;
    std::vector<double> rule_x, rule_w;       // the tensor rule on the unit cell (full cells)
    long long ncut = 0, nnodes = 0, nfull = 0, nfallback = 0;
    double cell_volume = 1.0;
    int ndim = 0;
    hipStream_t stream = nullptr;
};

// Gauss–Legendre on [0, 1], ascending: Newton on P_q in long double
static void quad_gauss(int q, double* x, double* w) {
    for (int i = 0; i < q; ++i) {
        long double z = cosl(3.14159265358979323846264338327950288L * (i + 0.75L) / (q + 0.5L)), dp = 1;
        for (int it = 0; it < 100; ++it) {
            long double p0 = 1, p1 = z;
            for (int m = 2; m <= q; ++m) { const long double p2 = ((2 * m - 1) * z * p1 - (m - 1) * p0) / m; p0 = p1; p1 = p2; }
            if (q == 1) { p1 = z; p0 = 1; }
            dp = q * (z * p1 - p0) / (z * z - 1);
            const long double dz = p1 / dp;
            z -= dz;
            if (fabsl(dz) < 1e-19L) break;
        }
        long double p0 = 1, p1 = z;
        for (int m = 2; m <= q; ++m) { const long double p2 = ((2 * m - 1) * z * p1 - (m - 1) * p0) / m; p0 = p1; p1 = p2; }
        dp = q * (z * p1 - p0) / (z * z - 1);
        x[i] = (double)((1 - z) / 2);                 // z descends with i
        w[i] = (double)(1 / ((1 - z * z) * dp * dp));   // 2 / ((1 - z²) P'²) on [-1, 1], halved
    }
}

template <int N, int NC>
static void quad_launch_cells(bool emit, const QuadArgs& qa, unsigned grid, hipStream_t st, const long long* cand, long long ncand, unsigned* counts,
                              const long long* node_off, const long long* pos, double* coords, double* weights, long long* cells, long long* offs,
                              unsigned* nfb) {
    if (emit) hipLaunchKernelGGL((quad_cells_kernel<N, NC, true>), dim3(grid), dim3(64), 0, st, qa, cand, ncand, counts, node_off, pos, coords, weights, cells, offs, nfb);
    else hipLaunchKernelGGL((quad_cells_kernel<N, NC, false>), dim3(grid), dim3(64), 0, st, qa, cand, ncand, counts, node_off, pos, coords, weights, cells, offs, nfb);
}
template <int N>
static void quad_launch_cells_n(int nc, bool emit, const QuadArgs& qa, unsigned grid, hipStream_t st, const long long* cand, long long ncand, unsigned* counts,
                                const long long* node_off, const long long* pos, double* coords, double* weights, long long* cells, long long* offs,
                                unsigned* nfb) {
#define QUAD_NC(NC_) case NC_: quad_launch_cells<N, NC_>(emit, qa, grid, st, cand, ncand, counts, node_off, pos, coords, weights, cells, offs, nfb); break;
    switch (nc) { QUAD_NC(2) QUAD_NC(3) QUAD_NC(4) QUAD_NC(5) QUAD_NC(6) }
#undef QUAD_NC
}

int quad_build(int ndim, const int n[3], const int goff[3], long long s1, long long s2, long long origin, const double lc[3], const double h[3],
               int order, int q, int surface, const void* phi, int f32, const unsigned char* mask, hipStream_t stream, QuadObject** out,
               long long counts_out[4], const char** err) {
    if (order < 1 || order > 5) { *err = "quadrature: interpolation_order must be in 1..5"; return 1; }
    if (q < 1 || q > QUAD_QMAX) { *err = "quadrature: quadrature_order must be in 1..20"; return 1; }
    QuadArgs qa;
    if (int r = setup_args(qa.a, ndim, n, goff, s1, s2, origin, lc, h, order, 1, 1, 0.0, 0.0, phi, f32, mask, err, true)) return r;
    for (int d = 0; d < ndim; ++d)
        if (n[d] < 2) { *err = "quadrature: at least two nodes per dimension"; return 1; }
    qa.q = q;
    qa.surface = surface ? 1 : 0;
    for (int i = 0; i < QUAD_QMAX; ++i) qa.gx[i] = qa.gw[i] = 0.0;
    quad_gauss(q, qa.gx, qa.gw);
    const ReinitArgs& a = qa.a;
    const int nc = order + 1;
    long long ncell = 1;
    for (int d = 0; d < ndim; ++d) ncell *= n[d] - 1;
    const long long nchunk = (ncell + QUAD_CHUNK - 1) / QUAD_CHUNK;

    std::unique_ptr<QuadObject> o(new QuadObject());
    o->ndim = ndim;
    o->stream = stream;
    for (int d = 0; d < ndim; ++d) o->cell_volume *= h[d];
    DevBuf<unsigned char> cls;
    DevBuf<unsigned> cnt;            // [cut | full] per chunk, then the node count per candidate cell
    DevBuf<long long> off, tot;      // scanned offsets; totals {cut, full, nodes, cut cells with nodes}
    DevBuf<long long> cand, node_off, pos;
    DevBuf<unsigned> nfb;
    MOD_HIP(cls.alloc((size_t)ncell), "hipMalloc(cell classes)");
    MOD_HIP(cnt.alloc(2 * (size_t)nchunk * sizeof(unsigned)), "hipMalloc(chunk counts)");
    MOD_HIP(off.alloc(2 * (size_t)nchunk * sizeof(long long)), "hipMalloc(chunk offsets)");
    MOD_HIP(tot.alloc(4 * sizeof(long long)), "hipMalloc(totals)");
    MOD_HIP(nfb.alloc(sizeof(unsigned)), "hipMalloc(fallback count)");
    MOD_HIP(hipMemsetAsync(nfb, 0, sizeof(unsigned), stream), "fallback count");
    // 1. classify, scan of the chunk counts
    const unsigned gchunk = (unsigned)nchunk;
#define QUAD_CLS(NV_, NC_, ND_) hipLaunchKernelGGL((quad_classify_kernel<NV_, NC_, ND_>), dim3(gchunk), dim3(256), 0, stream, qa, ncell, cls.p, cnt.p, cnt.p + nchunk)
    if (a.nv <= 4) {
        if (ndim == 1) { if (nc == 2) QUAD_CLS(2, 2, 1); else if (nc == 3) QUAD_CLS(4, 3, 1); else QUAD_CLS(4, 4, 1); }
        else if (ndim == 2) { if (nc == 2) QUAD_CLS(2, 2, 2); else if (nc == 3) QUAD_CLS(4, 3, 2); else QUAD_CLS(4, 4, 2); }
        else { if (nc == 2) QUAD_CLS(2, 2, 3); else if (nc == 3) QUAD_CLS(4, 3, 3); else QUAD_CLS(4, 4, 3); }
    } else {
        if (ndim == 1) QUAD_CLS(0, 0, 1); else if (ndim == 2) QUAD_CLS(0, 0, 2); else QUAD_CLS(0, 0, 3);
    }
#undef QUAD_CLS
    chunk_scan<2, long long>(stream, {{{cnt.p, off.p, 0}, {cnt.p + nchunk, off.p + nchunk, 0}}}, nchunk, tot.p);
    long long th[4] = {0, 0, 0, 0};
    MOD_HIP(hipMemcpyAsync(th, tot, 2 * sizeof(long long), hipMemcpyDeviceToHost, stream), "cell counts");
    MOD_HIP(hipStreamSynchronize(stream), "cell counts");
    const long long ncand = th[0];
    o->nfull = th[1];
    // 2. the ordered lists of candidate cut cells and of full cells
    MOD_HIP(cand.alloc((size_t)std::max(ncand, 1LL) * sizeof(long long)), "hipMalloc(cut cells)");
    MOD_HIP(o->full.alloc((size_t)std::max(o->nfull, 1LL) * sizeof(long long)), "hipMalloc(full cells)");
    hipLaunchKernelGGL(quad_compact_kernel, dim3(gchunk), dim3(256), 0, stream, cls.p, ncell, off.p, off.p + nchunk, cand.p, o->full.p);
    // 3. nodes per cut cell, scanned: node offsets and the slots of the cells that have nodes
    MOD_HIP(cnt.grow((size_t)std::max(ncand, 1LL) * sizeof(unsigned)), "hipMalloc(node counts)");
    MOD_HIP(node_off.alloc((size_t)std::max(ncand, 1LL) * sizeof(long long)), "hipMalloc(node offsets)");
    MOD_HIP(pos.alloc((size_t)std::max(ncand, 1LL) * sizeof(long long)), "hipMalloc(cell slots)");
    const unsigned gcell = (unsigned)std::min<long long>(std::max(ncand, 1LL), 1LL << 20);
#define QUAD_CELLS(EMIT_, ...) do { \
        if (ndim == 1) quad_launch_cells_n<1>(nc, EMIT_, qa, gcell, stream, cand, ncand, cnt, node_off, pos, __VA_ARGS__, nfb); \
        else if (ndim == 2) quad_launch_cells_n<2>(nc, EMIT_, qa, gcell, stream, cand, ncand, cnt, node_off, pos, __VA_ARGS__, nfb); \
        else quad_launch_cells_n<3>(nc, EMIT_, qa, gcell, stream, cand, ncand, cnt, node_off, pos, __VA_ARGS__, nfb); } while (0)
    if (ncand) QUAD_CELLS(false, nullptr, nullptr, nullptr, nullptr);
    chunk_scan<2, long long>(stream, {{{cnt.p, node_off.p, 0}, {cnt.p, pos.p, 1}}}, ncand, tot.p + 2);      // pos: the scan of count != 0
    unsigned hfb = 0;
    MOD_HIP(hipMemcpyAsync(th + 2, tot.p + 2, 2 * sizeof(long long), hipMemcpyDeviceToHost, stream), "node counts");
    MOD_HIP(hipMemcpyAsync(&hfb, nfb, sizeof(unsigned), hipMemcpyDeviceToHost, stream), "node counts");
    MOD_HIP(hipStreamSynchronize(stream), "node counts");
    o->nnodes = th[2];
    o->ncut = th[3];
    o->nfallback = hfb;
    // 4. the nodes
    MOD_HIP(o->cells.alloc((size_t)std::max(o->ncut, 1LL) * sizeof(long long)), "hipMalloc(cells)");
    MOD_HIP(o->offsets.alloc((size_t)(o->ncut + 1) * sizeof(long long)), "hipMalloc(offsets)");
    MOD_HIP(o->coords.alloc((size_t)std::max(o->nnodes, 1LL) * ndim * sizeof(double)), "hipMalloc(coords)");
    MOD_HIP(o->weights.alloc((size_t)std::max(o->nnodes, 1LL) * sizeof(double)), "hipMalloc(weights)");
    MOD_HIP(o->sum.alloc(sizeof(double)), "hipMalloc(sum)");
    if (o->ncut) QUAD_CELLS(true, o->coords.p, o->weights.p, o->cells.p, o->offsets.p);
#undef QUAD_CELLS
    MOD_HIP(hipMemcpyAsync(o->offsets.p + o->ncut, &o->nnodes, sizeof(long long), hipMemcpyHostToDevice, stream), "offsets");
    MOD_HIP(hipGetLastError(), "quadrature: launch failed");
    MOD_HIP(hipStreamSynchronize(stream), "quadrature: device error");
    // the tensor rule of a full cell on [0, 1]^N, in the order and with the products of the device's tensor rule
    int m = 1;
    for (int d = 0; d < ndim; ++d) m *= q;
    o->rule_x.assign((size_t)m * ndim, 0.0);
    o->rule_w.assign((size_t)m, 1.0);
    for (int p = 0; p < m; ++p) {
        double w = 1.0;
        for (int d = 0, r = p; d < ndim; ++d) {      // the last axis fastest
            const int sh = ndim - 1 - d;
            int div = 1;
            for (int e = 0; e < sh; ++e) div *= q;
            const int i = (r / div) % q;
            o->rule_x[(size_t)p * ndim + d] = 0.0 + (0.0 + (1.0 - 0.0) * qa.gx[i]) * 1.0;
            w = w * ((1.0 - 0.0) * qa.gw[i] * 1.0);
        }
        o->rule_w[p] = w;
    }
    counts_out[0] = o->ncut; counts_out[1] = o->nnodes; counts_out[2] = o->nfull; counts_out[3] = o->nfallback;
    *out = o.release();
    return 0;
}

int quad_read(QuadObject* o, long long* cells, long long* offsets, double* coords, double* weights, long long* full, double* rule_x, double* rule_w,
              const char** err) {
    hipError_t e = hipSuccess;
    auto cp = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind k) {
        if (dst && bytes && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, k, o->stream);
    };
    cp(cells, o->cells, (size_t)o->ncut * sizeof(long long), hipMemcpyDeviceToDevice);
    cp(offsets, o->offsets, (size_t)(o->ncut + 1) * sizeof(long long), hipMemcpyDeviceToDevice);
    cp(coords, o->coords, (size_t)o->nnodes * o->ndim * sizeof(double), hipMemcpyDeviceToDevice);
    cp(weights, o->weights, (size_t)o->nnodes * sizeof(double), hipMemcpyDeviceToDevice);
    cp(full, o->full, (size_t)o->nfull * sizeof(long long), hipMemcpyDeviceToDevice);
    cp(rule_x, o->rule_x.data(), o->rule_x.size() * sizeof(double), hipMemcpyHostToDevice);
    cp(rule_w, o->rule_w.data(), o->rule_w.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) { *err = "quadrature read: device error"; return 2; }
    return 0;
}

int quad_total(QuadObject* o, double* total, const char** err) {
    hipLaunchKernelGGL(quad_sum_kernel, dim3(1), dim3(1024), 0, o->stream, o->weights.p, o->nnodes, o->sum.p);
    double s = 0.0;
    hipError_t e = hipMemcpyAsync(&s, o->sum, sizeof(double), hipMemcpyDeviceToHost, o->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) { *err = "quadrature total: device error"; return 2; }
    double rs = 0.0;
    for (double w : o->rule_w) rs += w;
    *total = s + (double)o->nfull * rs * o->cell_volume;
    return 0;
}

void quad_free(QuadObject* o) { delete o; }
