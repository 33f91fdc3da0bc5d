// lsm_handle.h — the handle behind the C ABI (include/lsm.h), shared by lsm_api.hip and lsm_comm.hip, and the owners of the
// host side's device and pinned buffers.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "lsm_internal.h"

namespace lsm {
// a device buffer that only grows: re-allocated when a call needs more than it holds (the set of a NewtonSDF object is built once;
// the workspace of reinitialize! lives on the handle and stops allocating after the first calls).  Frees itself.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;            // bytes
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    operator T*() const { return p; }
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    hipError_t grow(size_t bytes) { return p && cap >= bytes ? hipSuccess : alloc(bytes + bytes / 4 + 256); }   // headroom: the band's size drifts
    void release() { (void)hipFree(p); p = nullptr; cap = 0; }
};
// its pinned-host twin (hipHostMalloc with the given flags)
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t cap = 0;            // bytes
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~PinnedBuf() { release(); }
    operator T*() const { return p; }
    hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
        release();
        const hipError_t e = hipHostMalloc((void**)&p, bytes, flags);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() { (void)hipHostFree(p); p = nullptr; cap = 0; }
};

struct I2oeWorkspace;   // lsm_i2oe.hip: SemiImplicitI2OE's device buffers
struct SemilagWorkspace;   // lsm_semilag.hip: SemiLagrangian's counters
struct MdistWorkspace;  // lsm_mdist.hip: mesh_distance's scratch arrays
struct EikonalWorkspace;   // lsm_eikonal.hip: eikonal's arrival times, frozen mask and tile lists
struct CcWorkspace;     // lsm_cc.hip: components' parent array, chunk counts and counters
struct NuWorkspace;     // lsm_nucleate.hip: nucleation's window keys, chunk counts and counters
}  // namespace lsm
struct LsmComm;   // lsm_comm.hip: slab communicator (RCCL or in-process), NULL on a single-device handle

struct LsmHandle {
    ~LsmHandle();        // lsm_api.hip: streams, events and workspaces; safe on a partly built handle
    LsmGrid grid;
    LsmBc bc[LSM_MAX_DIM][2];
    LsmSlab slab;
    int dtype, mode, device;
    LsmLayout lay;
    int nloc[3], goff[3], gn[3];
    double h[3], h2[3], inv_h[3], inv_h2[3], dxmin;
    double w[3][2][LSM_GHOST][8];
    hipStream_t stream = nullptr;
    bool own_stream = false;
    lsm::DevBuf<double> d_w;             // device copy of w
    lsm::DevBuf<signed char> d_ring;     // narrow band: distance-sorted offset ring
    int nring = 0;
    int nring_lds = 0;   // ring entries before the first with a component beyond the LDS apron (3)
    lsm::DevBuf<int> d_miss;
    lsm::DevBuf<unsigned long long> d_count;
    lsm::DevBuf<unsigned char> d_work;        // per-tile work flags (narrow band)
    lsm::DevBuf<unsigned char> d_tiles_old;   // the old band's tile flags during an update (the new ones are written in place)
    const unsigned char* band_mask = nullptr;   // set for the duration of a *_band call
    const unsigned char* band_tiles = nullptr;
    int band_mc = 0;
    const int* band_list = nullptr;    // compact active-tile list for a stage (NULL = flags only)
    unsigned band_nlist = 0;
    // compact tile lists of the band last updated (built on the device by lsm_band_update, lengths read back by
    // lsm_band_status): with them the band kernels launch one block per listed tile instead of one per tile
    lsm::DevBuf<int> d_act_list;
    lsm::DevBuf<int> d_work_list;
    lsm::DevBuf<unsigned> d_lcounts;
    const void* lists_tiles = nullptr; // the tile-flag buffer the lists describe
    int lists_mc = 0;
    bool lists_host_valid = false;
    const void* halo_n_key = nullptr;  // the device counter whose value lsm_band_status last read (NULL: unknown on the host)
    long long halo_n = 0;
    unsigned nact = 0, nwork = 0, nface = 0;   // list lengths; work tiles on a face of the grid
    lsm::LsmTuning tune;               // tuning switches: the environment's (read once per process) unless lsm_set_tuning changed them
    bool no_lists;                     // = tune.band_no_lists: always launch over all tiles
    bool band_bytes;                   // = tune.band_bytes: byte-mask band kernels in 3-D too
    lsm::DevBuf<double> d_partial;     // 2 * MAXB doubles
    lsm::DevBuf<int> d_flag;
    lsm::DevBuf<double> d_result;      // 16 doubles: [0..1] reductions, [2..6] lsm_band_status, [8..11] Δt of the next step prefetched by lsm_band_update
    lsm::PinnedBuf<double> h_result;   // pinned and mapped, 16 doubles
    double* h_result_dev = nullptr;    // the same page as the device sees it: lsm_band_status's kernel writes its numbers there directly
    unsigned long long status_ticket = 0;   // lsm_band_status: the kernel's last store is the call's ticket ([13]); the host spins on it
    // Δt of a band, prefetched: when the terms of the last lsm_compute_cfl_band depend neither on t nor on a field (constants,
    // ROTATION, SEPARABLE without time factor, Eikonal), lsm_band_update runs their reductions over the NEW band right behind
    // its own kernels and lsm_band_status brings the results home in the read it does anyway — the next lsm_compute_cfl_band
    // with the same terms on the same band launches nothing and waits for nothing
    struct BandCfl {
        LsmTerm terms[LSM_MAX_TERMS];
        int nterms;
        const void *mask, *tiles;
        int mc;
        bool armed, pending, valid;
        int slot[LSM_MAX_TERMS];           // result slot of a node-dependent term, -1 otherwise
        double dt[LSM_MAX_TERMS];
    } band_cfl = {};
    lsm::DevBuf<int> d_pf_flag;        // NaN flags of the prefetched reductions (4)
    std::string err;
    bool cfl_cache_on = true;
    bool cfl_prefetched = false;   // set around lsm_compute_cfl by lsm_compute_cfl_band when band_cfl holds this call's values
    std::vector<std::pair<LsmTerm, double>> cfl_cache;   // time-independent analytic coefficients
    struct CflCand { LsmTerm key; lsm::DevBuf<long long> d_cand; unsigned count; };
    std::vector<CflCand> cfl_cand;                       // SEPARABLE × g(t): the arg-max candidates are time-independent
    lsm::DevBuf<unsigned> d_cand_count;
    // Δt of a ϕ-independent term (constant / catalogued analytic coefficient) is reduced on a stream of its own, with
    // its own scratch: the host gets it without waiting for the stages queued on the main stream, and can queue the
    // next step behind them
    hipStream_t cfl_stream = nullptr;
    lsm::DevBuf<double> c_partial, c_result;
    lsm::PinnedBuf<double> ch_result;
    lsm::DevBuf<int> c_flag;
    std::vector<const void*> cfl_seen;   // coefficient tables known to have landed
    bool prof = false;
    int prof_every = 1;          // lsm_profile_enable(h, N): every N-th stage launch is timed
    unsigned long long prof_seen = 0;   // stage launches since lsm_profile_enable / lsm_profile_read
    std::vector<hipEvent_t> ev_start, ev_stop;
    size_t ev_used = 0;
    lsm::ReinitWorkspace* reinit_ws = nullptr;   // reinitialize!'s device buffers, kept between calls (grow-only)
    lsm::I2oeWorkspace* i2oe_ws = nullptr;       // lsm_advance_i2oe's solver vectors and face arrays, kept between calls (grow-only)
    lsm::SemilagWorkspace* semilag_ws = nullptr; // lsm_advance_semilag's workgroup counters and their pinned copy
    lsm::MdistWorkspace* mdist_ws = nullptr;     // lsm_mesh_distance's squared distances and flip counters, kept between calls (grow-only)
    lsm::EikonalWorkspace* eikonal_ws = nullptr; // lsm_eikonal's arrival times, frozen mask, tile flags and lists, kept between calls (grow-only)
    lsm::CcWorkspace* cc_ws = nullptr;           // lsm_cc_*'s parent array (4 bytes per node), chunk counts and counters, kept between calls (grow-only)
    lsm::NuWorkspace* nu_ws = nullptr;           // lsm_nucleate_*'s window keys (24 bytes per node), chunk counts and counters, kept between calls (grow-only)
    LsmComm* comm = nullptr;       // multi-GPU: attached by lsm_comm_attach_* (slab handles)
    bool yredirect = false;        // ... and those of dimension 2 (3-D)
    bool mredirect = false;        // ... and the march axis' NeumannBC faces are served by clamping the march at the boundary plane: no fill is left
    int ghost_depth = LSM_GHOST;   // ghost layers the fills write and the slab exchange sends: LSM_GHOST, or what the step in progress reads (XRedirect)
    int slab_depth_valid = LSM_GHOST;   // slab steps: ghost layers of ϕ (boundary conditions + neighbours' planes) the last step left valid;
                                        // a slab's ghosts are the host's to make valid before its first step (include/lsm.h)
    lsm::DevBuf<unsigned> d_tail_ctr;   // ring of LSM_TAIL_SLOTS ticket counters of the dynamic tail (each launch resets its own)
    unsigned tail_ticket = 0;      // host: launches that took a slot so far
    bool xredirect = false;        // set around the stages of a whole-grid lsm_advance_*: x ghosts are resolved by the stage kernel's loads
    lsm::DevBuf<unsigned long long> d_stamp;   // diagnostic build (-DLSM_STAMP): 8192 x {Δs_memtime, Δs_memrealtime, start, end} of the stage kernel's workgroups
};

// shared helpers (lsm_api.hip)
int lsm_fail(LsmHandle* h, int code, const std::string& msg);

// ---- the host side's scaffolding, one definition each
// in a function of the C ABI: a failed HIP call returns LSM_ERR_HIP with the call's text and HIP's message on the handle
#define LSM_HIP(h, call)                                                                                          \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess) return lsm_fail(h, LSM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
// in a module function that returns 0, 1 (refused) or 2 (device error) and has a `const char** err`: a failed HIP call returns 2
// with *err = what.  Objects under construction are held by std::unique_ptr: nothing to release here.
#define MOD_HIP(call, what) do { if ((call) != hipSuccess) { *err = what; return 2; } } while (0)
// kernel<2> or kernel<3> by the number of dimensions
#define LSM_LAUNCH_ND(ndim, kernel, grid, block, stream, ...)                                              \
    do {                                                                                                   \
        if ((ndim) == 2) hipLaunchKernelGGL(kernel<2>, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);   \
        else hipLaunchKernelGGL(kernel<3>, dim3(grid), dim3(block), 0, stream, __VA_ARGS__);               \
    } while (0)

// lsm_comm.hip: the attached communicator wants boundary-first stages (lsm_comm_set_overlap; LSM_SLAB_OVERLAP=0 at attach time)
bool lsm_comm_overlap(const LsmHandle* h);
int lsm_host_sync(LsmHandle* h, const char* what);   // host wait for h->stream that an RCCL peer's silence cannot hang (lsm_comm.hip)
int lsm_comm_band_overlap(const LsmHandle* h);   // overlap depth declared by lsm_band_overlap_config (0 = none)
namespace lsm { void i2oe_workspace_free(I2oeWorkspace* w); }   // lsm_i2oe.hip: delete, where the type is complete
namespace lsm { void semilag_workspace_free(SemilagWorkspace* w); }   // lsm_semilag.hip: delete, where the type is complete
namespace lsm {   // lsm_quad.hip (compiled through lsm_reinit.hip): quadrature results
struct QuadObject;
int quad_build(int ndim, const int n[3], const int goff[3], long long s1, long long s2, long long origin, const double lc[3], const double h[3],
               int order, int q, int surface, const void* phi, int f32, const unsigned char* mask, hipStream_t stream, QuadObject** out,
               long long counts_out[4], const char** err);
int quad_read(QuadObject* o, long long* cells, long long* offsets, double* coords, double* weights, long long* full, double* rule_x, double* rule_w,
              const char** err);
int quad_total(QuadObject* o, double* total, const char** err);
void quad_free(QuadObject* o);
}
namespace lsm {   // lsm_iso.hip: interface meshes (the geometry comes from the handle's grid and layout)
struct IsoObject;
int iso_build(const LsmHandle* h, double level, const void* phi, const unsigned char* mask, IsoObject** out, long long counts_out[2], const char** err);
int iso_read(IsoObject* o, double* verts, long long* elems, const char** err);
void iso_free(IsoObject* o);
}
namespace lsm {   // lsm_vol.hip: meshes of the interior
struct VolObject;
int vol_build(const LsmHandle* h, double level, const void* phi, VolObject** out, long long counts_out[3], const char** err);
int vol_read(VolObject* o, double* verts, long long* elems, long long* iface, const char** err);
void vol_free(VolObject* o);
}
namespace lsm {   // lsm_render.hip: pictures of the interface
struct RenderObject;
int render_build(int ndim, const int n[3], long long s1, long long s2, long long origin, const double lc[3], const double hc[3], const double h[3],
                 double level, const void* phi, int f32, const unsigned char* mask, hipStream_t stream, RenderObject** out, const char** err);
int render_refresh(RenderObject* o, const char** err);
int render_draw(RenderObject* o, const double* cam, int W, int H, const double* style, int skip, unsigned char* rgba, void* depth_or_cls, double* normal,
                hipStream_t stream, const char** err);
int render_bricks(RenderObject* o, long long dims[3], unsigned char* table, const char** err);
void render_free(RenderObject* o);
}
namespace lsm {   // lsm_mdist.hip: from a mesh back to a level set
int mdist_run(int ndim, const int n[3], long long s1, long long s2, long long origin, const double lc[3], const double h[3], long long nv,
              const double* verts, long long ne, const long long* elems, double cutoff, void* phi, int f32, hipStream_t stream, long long stats[3],
              const char** err, MdistWorkspace** workspace);
void mdist_workspace_free(MdistWorkspace* w);   // delete, where the type is complete
}
namespace lsm {   // lsm_eikonal.hip: |∇T| = 1/F over the whole grid by the block-based fast iterative method
int eikonal_run(int ndim, const int n[3], long long s1, long long s2, long long origin, const double h[3], void* phi, int f32, const double* speed,
                double width, double cutoff, long long max_iters, hipStream_t stream, long long stats[4], const char** err, EikonalWorkspace** workspace);
void eikonal_workspace_free(EikonalWorkspace* w);   // delete, where the type is complete
int extend_run(int ndim, const int n[3], long long s1, long long s2, long long origin, const double h[3], const void* phi, int f32, void* const* F, int K,
               int rule, const unsigned char* mask, double width, int source, double cutoff, double fill, long long max_iters, hipStream_t stream,
               long long stats[5], const char** err, EikonalWorkspace** workspace);   // extend_from_interface_ on eikonal's tile lists
}
namespace lsm {   // lsm_cc.hip: connected components of {ϕ < level} or of its complement over the Kuhn edges, by block-based union–find
struct CcObject;
int cc_build(const LsmHandle* h, CcWorkspace** workspace, double level, int side, const void* phi, CcObject** out, long long stats[4], const char** err);
int cc_read(CcObject* o, int* labels, long long* nodes, long long* sums, int* bbox, const char** err);
int cc_flip(CcObject* o, CcWorkspace* w, void* phi, const unsigned char* which, long long* flipped, const char** err);
void cc_free(CcObject* o);
void cc_workspace_free(CcWorkspace* w);   // delete, where the type is complete
}
namespace lsm {   // lsm_nucleate.hip: the centres a criterion field selects by non-maximum suppression, and the punch of a ball around each
struct NuObject;
int nu_build(const LsmHandle* h, NuWorkspace** workspace, const void* phi, const void* t, double threshold, double level, double clearance, double spacing,
             NuObject** out, long long* count, const char** err);
int nu_read(NuObject* o, long long* indices, double* values, const char** err);
int nu_punch(const LsmHandle* h, NuWorkspace** workspace, void* phi, const long long* centres, long long count, double level, double radius, long long* changed,
             const char** err);
void nu_free(NuObject* o);
void nu_workspace_free(NuWorkspace* w);   // delete, where the type is complete
}
