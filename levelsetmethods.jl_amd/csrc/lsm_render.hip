// lsm_render.hip — render(ϕ, camera) on the device: what ext/MakieExt.jl:142-171 draws.  3-D: volume!(ϕ; algorithm = :iso,
// isovalue = level), the first hit of a ray march through the trilinear interpolant of the sampled field, shaded by the
// interpolant's gradient.  2-D: contourf! under contour! at the level, a band's active cells tinted.  tests/_render_ref.py
// restates every operation; DESIGN.md §7.13 has the rules and the argument for the skipping.  Everything is fp64, the object is
// built with -ffp-contract=off, and only + − × / sqrt, floor and comparisons touch a number that reaches an output.
// Kernels:
//   * render_brick_kernel: one wave per brick of 8³ cells, one lane per (x, y) column marching z over 9 node planes: a byte of
//     state per brick (void / all outside / all inside / mixed); a cell counts as outside or inside only with a margin of
//     10⁻⁶·max|corner| that covers the rounding of the lerps, so that every sample in such a cell has the cell's state;
//   * render_ring_kernel: a brick is uniform iff it is not mixed and its 3 × 3 × 3 neighbours in the grid have its state;
//   * render_ray_kernel: one thread per pixel, a wave an 8 × 8 tile, a workgroup 16 × 16.  Lattice samples t_k = t_in + k·dt; a
//     sample whose cell lies in a uniform brick has the brick's state without a load, and k moves to the last lattice index
//     before the ray leaves the brick (floor, no + 1, at least one forward).  Values are loaded in mixed bricks only, and again
//     at a bracket's ends when a neighbour of the hit was skipped.  No atomics, no LDS, no scratch;
//   * render_2d_kernel: one thread per pixel, the same cell loader.
#include <cmath>

#include "lsm_handle.h"
#include "wave.h"

namespace lsm {

constexpr int RB = 8;                      // cells per brick and axis
enum { R_VOID = 0, R_OUT = 1, R_IN = 2, R_MIXED = 3, R_UNIFORM = 4 };

struct RenderArgs {
    int n[3];
    long long s1, s2, origin;   // the padded layout of ϕ and of the band mask
    double lc[3], hc[3], h[3];
    double level;
    const void* phi;
    const unsigned char* mask;  // narrow band: 1 = band node (NULL = dense)
    int nb[3];                  // bricks per axis
    const unsigned char* table; // per brick: state | R_UNIFORM
};

struct RayArgs {
    double eye[3], fwd[3], rs[3], us[3];
    int ortho, W, H, bisections;
    double color[3], ambient, dt, inv_dt;
    unsigned char bg[3];
};

struct FlatArgs {
    int W, H;
    double x0, x1, y0, y1, half_lw_px;
    unsigned char tab[6][3];
    int band;
};

// the cell of a position: clamped index, unclamped weight
__device__ __forceinline__ void rcell(double p, double lc, double h, int n, int& c, double& w) {
    const double x = (p - lc) / h;
    double cf = floor(x);
    const double top = (double)(n - 2);
    cf = cf < 0.0 ? 0.0 : (cf > top ? top : cf);
    c = (int)cf;
    c = c < 0 ? 0 : (c > n - 2 ? n - 2 : c);     // a NaN position (refused on the host) must not index outside the grid
    w = x - cf;
}

// the 2^N corners of the cell at q (padded offset of its anchor); false if a corner is off the band (then v is not loaded)
template <int N, class T>
__device__ __forceinline__ bool rload(const RenderArgs& a, long long q, double v[1 << N]) {
    if (a.mask) {
        bool on = true;
#pragma unroll
        for (int m = 0; m < (1 << N); ++m)
            on = on && a.mask[q + (m & 1) + ((m & 2) ? a.s1 : 0) + (N > 2 && (m & 4) ? a.s2 : 0)] != 0;
        if (!on) return false;
    }
    const T* f = static_cast<const T*>(a.phi);
#pragma unroll
    for (int m = 0; m < (1 << N); ++m) v[m] = (double)f[q + (m & 1) + ((m & 2) ? a.s1 : 0) + (N > 2 && (m & 4) ? a.s2 : 0)];
    return true;
}

struct Sample3 {
    double val;
    bool active;     // every corner on the band (dense: always)
    long long q;
    double wx, wy, wz;
};

__device__ __forceinline__ double rlerp(double a, double b, double w) { return a + w * (b - a); }

__device__ __forceinline__ void rpos(const RenderArgs& a, const double o[3], const double d[3], double t, int c[3], double w[3]) {
#pragma unroll
    for (int e = 0; e < 3; ++e) rcell(o[e] + t * d[e], a.lc[e], a.h[e], a.n[e], c[e], w[e]);
}

template <class T>
__device__ __forceinline__ int rsample(const RenderArgs& a, const int c[3], const double w[3], double& val) {
    double v[8];
    const long long q = a.origin + c[0] + c[1] * a.s1 + c[2] * a.s2;
    if (!rload<3, T>(a, q, v)) { val = 0.0; return R_VOID; }
    const double c00 = rlerp(v[0], v[1], w[0]), c10 = rlerp(v[2], v[3], w[0]);
    const double c01 = rlerp(v[4], v[5], w[0]), c11 = rlerp(v[6], v[7], w[0]);
    val = rlerp(rlerp(c00, c10, w[1]), rlerp(c01, c11, w[1]), w[2]);
    return val != val ? R_VOID : (val < a.level ? R_IN : R_OUT);
}

template <class T>
__device__ __forceinline__ int rsample_at(const RenderArgs& a, const double o[3], const double d[3], double t, double& val) {
    int c[3];
    double w[3];
    rpos(a, o, d, t, c, w);
    return rsample<T>(a, c, w, val);
}

template <class T, bool SKIP>
__global__ void __launch_bounds__(256) render_ray_kernel(RenderArgs a, RayArgs r, unsigned char* rgba, double* depth, double* normal) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int j = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (i >= r.W || j >= r.H) return;
    const long long pix = (long long)j * r.W + i;
    const double sx = (2.0 * ((double)i + 0.5)) / (double)r.W - 1.0;
    const double sy = 1.0 - (2.0 * ((double)j + 0.5)) / (double)r.H;
    double o[3], d[3];
    if (r.ortho) {
#pragma unroll
        for (int e = 0; e < 3; ++e) { o[e] = (r.eye[e] + sx * r.rs[e]) + sy * r.us[e]; d[e] = r.fwd[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 3; ++e) { o[e] = r.eye[e]; d[e] = (r.fwd[e] + sx * r.rs[e]) + sy * r.us[e]; }
        const double nn = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
        for (int e = 0; e < 3; ++e) d[e] = d[e] / nn;
    }
    double tin = 0.0, tout = INFINITY;
    bool miss = false;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        if (d[e] == 0.0) {
            miss = miss || o[e] < a.lc[e] || o[e] > a.hc[e];
        } else {
            const double t1 = (a.lc[e] - o[e]) / d[e], t2 = (a.hc[e] - o[e]) / d[e];
            const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
            if (tn > tin) tin = tn;
            if (tf < tout) tout = tf;
        }
    }
    miss = miss || !(tout > tin && tout < INFINITY);

    bool hit = false;
    double th = INFINITY;
    if (!miss) {
        double inv_d[3];           // only the skip's length comes from these: never an output
#pragma unroll
        for (int e = 0; e < 3; ++e) inv_d[e] = 1.0 / d[e];
        double k = 0.0, pv = 0.0, ta = 0.0, tb = 0.0, va = 0.0, vb = 0.0;
        int pst = R_VOID;
        bool pknown = false, bracket = false;
        for (;;) {
            const double t = tin + k * r.dt;
            if (!(t <= tout)) break;
            int c[3];
            double w[3], val = 0.0, knext = k + 1.0;
            rpos(a, o, d, t, c, w);
            int st;
            bool known = true;
            const unsigned char bs = SKIP ? a.table[((long long)(c[2] >> 3) * a.nb[1] + (c[1] >> 3)) * a.nb[0] + (c[0] >> 3)] : (unsigned char)0;
            if (SKIP && (bs & R_UNIFORM)) {
                st = bs & 3;
                known = false;
                double te = INFINITY;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const int b = c[e] >> 3;
                    const int last = (b + 1) * RB < a.n[e] - 1 ? (b + 1) * RB : a.n[e] - 1;
                    const double face = a.lc[e] + (double)(d[e] > 0.0 ? last : b * RB) * a.h[e];
                    const double tf = d[e] != 0.0 ? (face - o[e]) * inv_d[e] : INFINITY;
                    if (tf < te) te = tf;
                }
                // the last lattice index before the exit face: the samples skipped, k + 1 .. kf − 1, end a whole dt short of it, which
                // the rounding of te cannot reach; sample kf is looked at like any other
                const double kf = floor((te - tin) * r.inv_dt);
                if (kf > knext) knext = kf;
            } else {
                st = rsample<T>(a, c, w, val);
            }
            if (k == 0.0 && st == R_IN) { hit = true; th = t; break; }
            if (k > 0.0 && pst != R_VOID && st != R_VOID && pst != st) {
                ta = tin + (k - 1.0) * r.dt;
                tb = t;
                if (pknown) va = pv; else (void)rsample_at<T>(a, o, d, ta, va);
                if (known) vb = val; else (void)rsample_at<T>(a, o, d, tb, vb);
                bracket = true;
                break;
            }
            pst = st;                                   // the state of sample knext − 1 too: the skipped samples share it
            pv = val;
            pknown = known;
            k = knext;
        }
        if (bracket) {
            const bool ina = va < a.level;
            for (int it = 0; it < r.bisections; ++it) {
                const double m = 0.5 * (ta + tb);
                double vm;
                const int sm = rsample_at<T>(a, o, d, m, vm);
                if (sm == R_VOID) break;
                if ((vm < a.level) == ina) { ta = m; va = vm; } else { tb = m; vb = vm; }
            }
            th = ta + ((a.level - va) / (vb - va)) * (tb - ta);
            hit = true;
        }
    }

    unsigned char px[4] = {r.bg[0], r.bg[1], r.bg[2], 255};
    double nrm[3] = {0.0, 0.0, 0.0};
    if (hit) {
        int c[3];
        double w[3], v[8];
        rpos(a, o, d, th, c, w);
        if (rload<3, T>(a, a.origin + c[0] + c[1] * a.s1 + c[2] * a.s2, v)) {
            const double c00 = rlerp(v[0], v[1], w[0]), c10 = rlerp(v[2], v[3], w[0]);
            const double c01 = rlerp(v[4], v[5], w[0]), c11 = rlerp(v[6], v[7], w[0]);
            const double c0 = rlerp(c00, c10, w[1]), c1 = rlerp(c01, c11, w[1]);
            const double dx00 = v[1] - v[0], dx10 = v[3] - v[2], dx01 = v[5] - v[4], dx11 = v[7] - v[6];
            const double gx = rlerp(rlerp(dx00, dx10, w[1]), rlerp(dx01, dx11, w[1]), w[2]) / a.h[0];
            const double gy = rlerp(c10 - c00, c11 - c01, w[2]) / a.h[1];
            const double gz = (c1 - c0) / a.h[2];
            const double nn = sqrt((gx * gx + gy * gy) + gz * gz);
            if (nn > 0.0) { nrm[0] = gx / nn; nrm[1] = gy / nn; nrm[2] = gz / nn; }
        }
        const double s = r.ambient + (1.0 - r.ambient) * fabs((nrm[0] * d[0] + nrm[1] * d[1]) + nrm[2] * d[2]);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const double q = floor(((255.0 * s) * r.color[e]) / 255.0 + 0.5);
            px[e] = (unsigned char)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
        }
    }
    if (rgba) *reinterpret_cast<uchar4*>(rgba + 4 * pix) = make_uchar4(px[0], px[1], px[2], px[3]);
    if (depth) depth[pix] = th;
    if (normal) { normal[3 * pix] = nrm[0]; normal[3 * pix + 1] = nrm[1]; normal[3 * pix + 2] = nrm[2]; }
}

template <class T>
__global__ void __launch_bounds__(256) render_2d_kernel(RenderArgs a, FlatArgs f, unsigned char* rgba, unsigned char* cls) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int j = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (i >= f.W || j >= f.H) return;
    const long long pix = (long long)j * f.W + i;
    const double X = f.x0 + (((double)i + 0.5) / (double)f.W) * (f.x1 - f.x0);
    const double Y = f.y1 - (((double)j + 0.5) / (double)f.H) * (f.y1 - f.y0);
    int cx, cy, k = 3;
    double wx, wy, v[4];
    rcell(X, a.lc[0], a.h[0], a.n[0], cx, wx);
    rcell(Y, a.lc[1], a.h[1], a.n[1], cy, wy);
    const bool off = X < a.lc[0] || X > a.hc[0] || Y < a.lc[1] || Y > a.hc[1];
    if (!off && rload<2, T>(a, a.origin + cx + cy * a.s1, v)) {
        const double c0 = rlerp(v[0], v[1], wx), c1 = rlerp(v[2], v[3], wx);
        const double val = rlerp(c0, c1, wy);
        const double gx = rlerp(v[1] - v[0], v[3] - v[2], wy) / a.h[0];
        const double gy = (c1 - c0) / a.h[1];
        const double nn = sqrt(gx * gx + gy * gy);
        if (val == val) k = fabs(val - a.level) <= f.half_lw_px * nn ? 2 : ((val < a.level ? 1 : 0) + (f.band ? 4 : 0));
    }
    if (rgba) *reinterpret_cast<uchar4*>(rgba + 4 * pix) = make_uchar4(f.tab[k][0], f.tab[k][1], f.tab[k][2], 255);
    if (cls) cls[pix] = (unsigned char)k;
}

// one wave per brick, four bricks along x per workgroup; lane (lx, ly) owns the column of cells (x, y, ·) of its brick and
// marches the 9 node planes: the extrema (and the band flags) of a plane's four nodes, combined with the previous plane's
template <class T>
__global__ void __launch_bounds__(256) render_brick_kernel(RenderArgs a, unsigned char* raw) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bx = blockIdx.x * 4 + wave, by = blockIdx.y, bz = blockIdx.z;
    if (bx >= a.nb[0]) return;                         // the whole wave
    const int x = bx * RB + (lane & 7), y = by * RB + (lane >> 3), z0 = bz * RB;
    const bool col = x < a.n[0] - 1 && y < a.n[1] - 1;
    const int z1 = z0 + RB < a.n[2] - 1 ? z0 + RB : a.n[2] - 1;     // last node plane of the brick
    const T* f = static_cast<const T*>(a.phi);
    unsigned seen = 0;
    if (col) {
        double pmn = 0.0, pmx = 0.0;
        bool pbad = false, pon = true;
        for (int z = z0; z <= z1; ++z) {
            const long long q = a.origin + x + y * a.s1 + z * a.s2;
            double mn = INFINITY, mx = -INFINITY;
            bool bad = false, on = true;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const long long qq = q + (m & 1) + ((m & 2) ? a.s1 : 0);
                const double v = (double)f[qq];
                bad = bad || v != v;
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
                if (a.mask) on = on && a.mask[qq] != 0;
            }
            if (z > z0) {
                int st = R_VOID;
                if (on && pon) {
                    const double cmn = pmn < mn ? pmn : mn, cmx = pmx > mx ? pmx : mx;
                    const double amn = fabs(cmn), amx = fabs(cmx), al = fabs(a.level);
                    double am = amn > amx ? amn : amx;
                    am = am > al ? am : al;
                    const double m = 1e-6 * am;
                    st = (bad || pbad) ? R_MIXED : (cmn > a.level + m ? R_OUT : (cmx < a.level - m ? R_IN : R_MIXED));
                }
                seen |= 1u << st;
            }
            pmn = mn; pmx = mx; pbad = bad; pon = on;
        }
    }
    seen = wave_or(seen);
    if (lane == 0) raw[((long long)bz * a.nb[1] + by) * a.nb[0] + bx] = (unsigned char)(__popc(seen) == 1 ? __ffs(seen) - 1 : R_MIXED);
}

__global__ void __launch_bounds__(256) render_ring_kernel(int nb0, int nb1, int nb2, const unsigned char* raw, unsigned char* table) {
    const long long nbrick = (long long)nb0 * nb1 * nb2;
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nbrick) return;
    const int bx = (int)(b % nb0), by = (int)((b / nb0) % nb1), bz = (int)(b / ((long long)nb0 * nb1));
    const unsigned char s = raw[b];
    bool uni = s != R_MIXED;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int X = bx + dx, Y = by + dy, Z = bz + dz;
                if (X < 0 || Y < 0 || Z < 0 || X >= nb0 || Y >= nb1 || Z >= nb2) continue;
                uni = uni && raw[((long long)Z * nb1 + Y) * nb0 + X] == s;
            }
    table[b] = (unsigned char)(s | (uni ? R_UNIFORM : 0));
}

// ---- host side
struct RenderObject {
    RenderArgs a;
    int ndim = 0, f32 = 0;
    long long nbrick = 0;
    DevBuf<unsigned char> raw, table;
    hipStream_t stream = nullptr;
};

int render_refresh(RenderObject* o, const char** err) {
    if (o->ndim != 3) return 0;
    const dim3 grid((unsigned)((o->a.nb[0] + 3) / 4), (unsigned)o->a.nb[1], (unsigned)o->a.nb[2]);
    if (o->f32) hipLaunchKernelGGL(render_brick_kernel<float>, grid, dim3(256), 0, o->stream, o->a, o->raw.p);
    else hipLaunchKernelGGL(render_brick_kernel<double>, grid, dim3(256), 0, o->stream, o->a, o->raw.p);
    hipLaunchKernelGGL(render_ring_kernel, dim3((unsigned)((o->nbrick + 255) / 256)), dim3(256), 0, o->stream, o->a.nb[0], o->a.nb[1], o->a.nb[2],
                       o->raw.p, o->table.p);
    if (hipGetLastError() != hipSuccess) { *err = "render: brick launch failed"; return 2; }
    return 0;
}

int render_build(int ndim, const int n[3], long long s1, long long s2, long long origin, const double lc[3], const double hc[3], const double h[3],
                 double level, const void* phi, int f32, const unsigned char* mask, hipStream_t stream, RenderObject** out, const char** err) {
    if (ndim != 2 && ndim != 3) { *err = "render: 2-D and 3-D fields only"; return 1; }
    RenderObject* o = new RenderObject();
    RenderArgs& a = o->a;
    o->nbrick = 1;
    for (int d = 0; d < 3; ++d) {
        a.n[d] = d < ndim ? n[d] : 2;
        a.lc[d] = d < ndim ? lc[d] : 0.0;
        a.hc[d] = d < ndim ? hc[d] : 1.0;
        a.h[d] = d < ndim ? h[d] : 1.0;
        if (d < ndim && n[d] < 2) { *err = "render: at least two nodes per dimension"; delete o; return 1; }
        a.nb[d] = (a.n[d] - 1 + RB - 1) / RB;
        o->nbrick *= a.nb[d];
    }
    a.s1 = s1; a.s2 = ndim > 2 ? s2 : 0; a.origin = origin;
    a.level = level; a.phi = phi; a.mask = mask; a.table = nullptr;
    o->ndim = ndim; o->f32 = f32; o->stream = stream;
    if (ndim == 3) {
        if (a.nb[1] > 65535 || a.nb[2] > 65535) { *err = "render: the grid has too many bricks"; delete o; return 1; }
        if (o->raw.alloc((size_t)o->nbrick) != hipSuccess || o->table.alloc((size_t)o->nbrick) != hipSuccess) {
            *err = "hipMalloc(bricks)"; delete o; return 2;
        }
        a.table = o->table.p;
        const int r = render_refresh(o, err);
        if (r) { delete o; return r; }
    }
    *out = o;
    return 0;
}

int render_draw(RenderObject* o, const double* cam, int W, int H, const double* style, int skip, unsigned char* rgba, void* depth_or_cls, double* normal,
                hipStream_t stream, const char** err) {
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16));
    if (grid.y > 65535) { *err = "render: the image is too high"; return 1; }
    if (o->ndim == 3) {
        RayArgs r;
        for (int e = 0; e < 3; ++e) {
            r.eye[e] = cam[e]; r.fwd[e] = cam[3 + e]; r.rs[e] = cam[6 + e]; r.us[e] = cam[9 + e];
            r.color[e] = style[e];
            r.bg[e] = (unsigned char)(style[3 + e] < 0.0 ? 0.0 : (style[3 + e] > 255.0 ? 255.0 : style[3 + e]));
        }
        r.ortho = cam[12] != 0.0; r.W = W; r.H = H;
        r.ambient = style[6];
        double hmin = o->a.h[0];
        for (int e = 1; e < 3; ++e) hmin = o->a.h[e] < hmin ? o->a.h[e] : hmin;
        r.dt = style[7] * hmin;
        r.inv_dt = 1.0 / r.dt;
        r.bisections = (int)style[8];
#define RENDER_RAY(T, S) hipLaunchKernelGGL((render_ray_kernel<T, S>), grid, dim3(256), 0, stream, o->a, r, rgba, (double*)depth_or_cls, normal)
        if (o->f32) { if (skip) RENDER_RAY(float, true); else RENDER_RAY(float, false); }
        else { if (skip) RENDER_RAY(double, true); else RENDER_RAY(double, false); }
#undef RENDER_RAY
    } else {
        FlatArgs f;
        f.W = W; f.H = H;
        f.x0 = style[1]; f.x1 = style[2]; f.y0 = style[3]; f.y1 = style[4];
        const double pw = (f.x1 - f.x0) / (double)W, ph = (f.y1 - f.y0) / (double)H;
        f.half_lw_px = (0.5 * style[0]) * (pw > ph ? pw : ph);
        for (int k = 0; k < 6; ++k)
            for (int e = 0; e < 3; ++e) {
                const double c = style[5 + 3 * k + e];
                f.tab[k][e] = (unsigned char)(c < 0.0 ? 0.0 : (c > 255.0 ? 255.0 : c));
            }
        f.band = o->a.mask != nullptr;
        if (o->f32) hipLaunchKernelGGL(render_2d_kernel<float>, grid, dim3(256), 0, stream, o->a, f, rgba, (unsigned char*)depth_or_cls);
        else hipLaunchKernelGGL(render_2d_kernel<double>, grid, dim3(256), 0, stream, o->a, f, rgba, (unsigned char*)depth_or_cls);
    }
    if (hipGetLastError() != hipSuccess) { *err = "render: launch failed"; return 2; }
    return 0;
}

int render_bricks(RenderObject* o, long long dims[3], unsigned char* table, const char** err) {
    for (int d = 0; d < 3; ++d) dims[d] = o->ndim == 3 ? o->a.nb[d] : 0;
    if (!table || o->ndim != 3) return 0;
    if (hipMemcpyAsync(table, o->table.p, (size_t)o->nbrick, hipMemcpyDeviceToDevice, o->stream) != hipSuccess ||
        hipStreamSynchronize(o->stream) != hipSuccess) { *err = "render bricks: device error"; return 2; }
    return 0;
}

void render_free(RenderObject* o) { delete o; }

}  // namespace lsm
