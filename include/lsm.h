/*
 * lsm.h — C ABI of libhiplsm: the MI355X (gfx950) grid-update hot path of
 * LevelSetMethods.jl behind plain pointers and sizes.
 *
 * The reference has no FFI: its seam is Julia multiple dispatch on the field type
 * (AbstractMeshField interface, src/meshfield.jl:11-33).  The entry points below are what a
 * device-resident AbstractMeshField subtype would `ccall` from the methods the integrator
 * reaches the field through.  Each declaration cites the reference code whose
 * loop body it replaces.  No torch/HIP types appear in signatures; `stream` is a hipStream_t
 * passed as void* (NULL = the handle's own stream).
 *
 * Conventions
 *  - All field pointers are DEVICE pointers to arrays in the *padded layout* described by
 *    LsmLayout (column-major like Julia's Array, dim 1 fastest, LSM_GHOST ghost layers on each
 *    side of every used dimension).  The caller owns the memory (AMDGPU.jl ROCArray / torch
 *    tensor); the library borrows pointers for the duration of a call.
 *  - Every call returns LSM_OK (0) or a negative error code; lsm_last_error() gives the text.
 *    The library never throws or aborts.
 *  - Calls are asynchronous on the handle's stream unless documented otherwise; calls that
 *    return a host value (lsm_compute_cfl, lsm_download) synchronise.
 */
#ifndef LSM_H
#define LSM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSM_MAX_DIM 3
#define LSM_GHOST 3          /* ghost layers per side: WENO5 needs 3 (src/derivatives.jl:89-121) */
#define LSM_MAX_TERMS 8

/* status codes */
enum {
    LSM_OK = 0,
    LSM_ERR_INVALID = -1,    /* bad argument / unsupported combination */
    LSM_ERR_HIP = -2,        /* a HIP runtime call failed */
    LSM_ERR_NO_DEVICE = -3,
    LSM_ERR_COMM = -4,       /* multi-GPU: a peer rank left / aborted / did not answer in time, or RCCL failed; the
                                communicator stays failed (lsm_comm_detach + a new attach to go on) */
    LSM_ERR_NOT_CONVERGED = -5   /* an iterative solve (lsm_advance_i2oe) broke down or did not reach its tolerance */
};

/* CartesianGrid (src/meshes.jl:1-5): lower/upper corner and node counts of the GLOBAL grid.
 * meshsize h_d = (hc_d - lc_d)/(n_d - 1) (src/meshes.jl:109-110). */
typedef struct LsmGrid {
    int32_t ndim;                 /* 1, 2 or 3 */
    int32_t _pad;
    int64_t n[LSM_MAX_DIM];       /* unused dims must be 1 */
    double lc[LSM_MAX_DIM];
    double hc[LSM_MAX_DIM];
} LsmGrid;

/* BoundaryCondition kinds (src/boundaryconditions.jl:27,40-46,63).  LSM_BC_NONE marks a slab
 * interface of a multi-GPU decomposition: its ghosts come from the halo exchange, the ghost
 * fill skips it. */
enum { LSM_BC_PERIODIC = 0, LSM_BC_EXTRAPOLATION = 1, LSM_BC_SYMMETRY = 2, LSM_BC_NONE = 3 };
typedef struct LsmBc {
    int32_t kind;
    int32_t degree;               /* P of ExtrapolationBC{P}; 0 = NeumannBC, 1 = LinearExtrapolationBC */
} LsmBc;

/* Slab of the last dimension owned by this handle (multi-GPU); lo is 0-based. */
typedef struct LsmSlab {
    int64_t lo;
    int64_t n;
} LsmSlab;

/* Padded device layout of one scalar field. element(i1,i2,i3) (0-based LOCAL interior index,
 * ghosts at -LSM_GHOST..-1 and n..n+LSM_GHOST-1) lives at origin + i1 + i2*stride[1] + i3*stride[2]. */
typedef struct LsmLayout {
    int64_t n[LSM_MAX_DIM];       /* local interior extent */
    int64_t g[LSM_MAX_DIM];       /* ghost width per dim (0 for unused dims) */
    int64_t stride[LSM_MAX_DIM];  /* stride[0] == 1 */
    int64_t origin;               /* offset of interior node (0,0,0) */
    int64_t total;                /* elements to allocate */
} LsmLayout;

/* LevelSetTerm kinds (src/levelsetterms.jl:45,104,139,211) and SpatialScheme (src/derivatives.jl:11,20) */
enum { LSM_TERM_ADVECTION = 0, LSM_TERM_NORMAL_MOTION = 1, LSM_TERM_CURVATURE = 2, LSM_TERM_EIKONAL = 3 };
enum { LSM_SCHEME_UPWIND = 0, LSM_SCHEME_WENO5 = 1 };

/* Coefficient of a term (velocity / speed / b), the device-side counterpart of
 * _eval_field (src/levelsetterms.jl:42-43).  Julia closures cannot run on the device, so:
 *   CONST      value[c]                                         (e.g. (x,t)->SVector(1.0))
 *   ROTATION   u1 = -(w*(x2-c2)), u2 = w*(x1-c1), u3 = 0         with w=value[0], c=value[1..2]
 *   SEPARABLE  u_c = ((T_c1[i1]*T_c2[i2])*T_c3[i3]) * g(t)       tables on the device, GLOBAL index;
 *              sep[c] points to the n1+n2+n3 concatenated doubles of component c
 *              g(t) = 1 (time_kind 0) or cos(pi*t/time_param) (time_kind 1)
 *   FIELD      field[c] = padded device array (same layout as phi), read in-grid only
 * Node coordinates are x_d = lc_d + i_d*h_d (src/meshes.jl:114-117). */
enum { LSM_COEFF_CONST = 0, LSM_COEFF_ROTATION = 1, LSM_COEFF_SEPARABLE = 2, LSM_COEFF_FIELD = 3 };
enum { LSM_TIME_ONE = 0, LSM_TIME_COS = 1 };
typedef struct LsmCoeff {
    int32_t kind;
    int32_t time_kind;
    double time_param;
    double value[4];
    const void* field[LSM_MAX_DIM];
    const double* sep[LSM_MAX_DIM];
} LsmCoeff;

typedef struct LsmTerm {
    int32_t kind;                 /* LSM_TERM_* */
    int32_t scheme;               /* LSM_SCHEME_* (advection only) */
    LsmCoeff coeff;               /* velocity (ndim comps) / speed / b (1 comp); unused for Eikonal */
    const void* s0;               /* Eikonal frozen sign field S0 (padded, src/levelsetterms.jl:217-221) or NULL */
} LsmTerm;

/* How a stage forms its base value before subtracting the terms (src/timestepping.jl:126-202):
 *   PSI     base = psi[I]                          (FE, RK2 predictor, RK3 stage 1; :129,:147,:172)
 *   RK3_S2  base = 0.75*phin[I] + 0.25*psi[I]      (:182)
 *   RK3_S3  base = (phin[I] + 2*psi[I]) / 3        (:193)
 *   OTHER   base = phin[I]                         (RK2 corrector accumulates onto corr; :160)
 */
enum { LSM_BASE_PSI = 0, LSM_BASE_RK3_S2 = 1, LSM_BASE_RK3_S3 = 2, LSM_BASE_OTHER = 3 };

/* arithmetic mode (lsm_create flags) */
enum {
    LSM_MODE_FAST = 0,    /* default: reciprocal-based divisions, FMA contraction, fused WENO weights;
                             within 1e-13*max|phi| of the reference arithmetic per stage */
    LSM_MODE_STRICT = 1   /* literal reference operation order, IEEE division, no contraction */
};
/* Domain of LSM_MODE_FAST (the 1e-13 bound above holds inside it):
 *  - differences between neighbouring nodes must stay below 1e35 in magnitude: the WENO5 weights are formed as products
 *    of squared smoothness indicators with ONE reciprocal (src/derivatives.jl:73-78 divides six times), which leave the
 *    fp64 range beyond that and produce Inf/NaN.  LSM_FAST_MAX_ABS bounds |phi| so that no difference can get there;
 *    lsm_check_range tests a field against it (the host layers call it when an equation is built and every 64 steps, and
 *    refuse to go on: rescale the field or create the handle with LSM_MODE_STRICT, which has no such limit).
 *  - the floor of the WENO5 regularisation eps = 1e-6*max(v_k^2) + 1e-99 (src/derivatives.jl:72) is, in undivided
 *    differences, 1e-99*h^2; FAST raises it to 1e-75 so that the weight denominator needs no guard.  Results change only
 *    where all five differences of a stencil are below ~3e-35, and there by less than those differences: a deviation
 *    from the reference by design, far inside the tolerance; exactly flat data gives exactly 0 in both modes.
 *  - an advection velocity component u_d = +0.0 takes the left-biased stencil where the reference takes the right-biased
 *    one; the term is |0|*W = 0 either way (a NaN velocity gives NaN in both). */
#define LSM_FAST_MAX_ABS 2.5e34
/* storage type of the level-set fields of a handle (ϕ, stage buffers, extension targets).  LSM_DTYPE_F32 is a
 * storage format only: values widen exactly on load, every computation is fp64, results are rounded to nearest
 * on store (the reference's Float32 fields compute in mixed Float32/Float64 by Julia's promotion rules; its
 * results differ from the fp64 ones by O(1e-7) relative, and so do these).  Coefficient fields, frozen signs and
 * frozen masks ("side arrays") are fp64 for either dtype, and so is every reduction. */
enum { LSM_DTYPE_F64 = 0, LSM_DTYPE_F32 = 1 };

typedef struct LsmHandle LsmHandle;

/* Host callback run between stage launches so host-side update_func hooks keep their
 * (stage field, stage time) semantics (src/timestepping.jl:131,149,158,174,185,196).
 * Called with the stream synchronised. Return non-zero to abort the step. */
typedef int (*LsmStageHook)(void* user, int stage, const void* stage_field, double stage_time);

/* ---- lifetime (LevelSetEquation construction, src/levelsetequation.jl:59-78) ---- */
int lsm_create(const LsmGrid* grid, const LsmBc bc[LSM_MAX_DIM][2], const LsmSlab* slab /* NULL = whole grid */,
               int dtype, int mode, int device, LsmHandle** out);
void lsm_destroy(LsmHandle* h);
const char* lsm_last_error(const LsmHandle* h /* NULL = creation errors */);
const char* lsm_version(void);
int lsm_sync(LsmHandle* h);
/* adopt the stream the caller's array library works on (hipStream_t as void*; the handle owns
 * a non-blocking stream of its own until this is called) */
int lsm_set_stream(LsmHandle* h, void* stream);

/* ---- layout + transfers (MeshField <-> device field; values(ϕ), src/meshfield.jl:58) ---- */
int lsm_layout(const LsmHandle* h, LsmLayout* out);
int lsm_upload(LsmHandle* h, void* dev_padded, const void* host_dense);     /* interior only; synchronous */
int lsm_download(LsmHandle* h, const void* dev_padded, void* host_dense);   /* interior only; synchronous */
/* the same for the fp64 side arrays of a handle of either dtype (host dense array of double) */
int lsm_upload_f64(LsmHandle* h, void* dev_padded, const void* host_dense);
int lsm_download_f64(LsmHandle* h, const void* dev_padded, void* host_dense);

/* ---- ghost resolution: _getindexbc + bc_stencil (src/meshfield.jl:248-260,
 *      src/boundaryconditions.jl:107-153) materialised into the ghost layers, dim 1 -> dim N.
 *      dim_mask bit d fills dimension d+1 (7 = all). */
int lsm_fill_ghosts(LsmHandle* h, void* field, int dim_mask, void* stream);

/* ---- one loop body of _advance! (src/timestepping.jl:128-137,143-164,170-202), all terms fused:
 *      out[I]  = (base - cdt*L_1(psi)[I]) - cdt*L_2(psi)[I] ...
 *      out2[I] = (psi[I] - cdt2*L_1) - cdt2*L_2 ...   (RK2's corr accumulator; NULL to skip)
 *      psi needs valid ghosts; out/out2 ghosts are NOT filled. out may alias phin (pointwise).
 *      One padded plane of the field (the whole array in 1-D, a row in 2-D) must be smaller than 2 GiB: the kernel
 *      addresses a plane through a buffer descriptor (LSM_ERR_INVALID otherwise). */
int lsm_stage(LsmHandle* h, const LsmTerm* terms, int nterms, const void* psi, const void* phin,
              void* out, void* out2, int base_mode, double cdt, double cdt2, double t_stage, void* stream);

/* The same two calls restricted to planes [m_begin, m_end) of the LAST dimension, so a slab can
 * update and ghost-fill its boundary planes first, start the halo exchange, and update the interior
 * while the planes travel (ndim >= 2).  lsm_fill_ghosts_planes fills the ghosts of dimensions
 * 1..N-1 on those planes and, if fill_last != 0, the physical (non-NONE) ghost planes of dimension N. */
int lsm_stage_planes(LsmHandle* h, const LsmTerm* terms, int nterms, const void* psi, const void* phin,
                     void* out, void* out2, int base_mode, double cdt, double cdt2, double t_stage,
                     int64_t m_begin, int64_t m_end, void* stream);
int lsm_fill_ghosts_planes(LsmHandle* h, void* field, int64_t m_begin, int64_t m_end, int fill_last, void* stream);

/* ---- compute_cfl (src/levelsetterms.jl:22-38,90-96,123-127,172-178,250).  *dt_out is the raw
 *      minimum (Inf, NaN and <=0 possible): the CALLER raises the reference's ArgumentError. */
int lsm_compute_cfl(LsmHandle* h, const LsmTerm* terms, int nterms, const void* phi, double t, double* dt_out);

/* The CFL of a catalogued analytic coefficient WITHOUT time factor (ROTATION, SEPARABLE with
 * LSM_TIME_ONE) is the same every step; it is computed once per handle and reused as long as the
 * LsmTerm is byte-identical.  Calling this (with 0 or 1) flushes the cache; pass 0 when table
 * contents are mutated in place between steps. */
int lsm_cfl_cache(LsmHandle* h, int enable);

/* ---- _advance! per integrator.  phi's ghost layers are (re)filled on entry; on return of a whole-grid handle they are
 *      STALE (the interior is the new state): every entry point that reads ghosts fills them itself, and a caller of
 *      lsm_stage calls lsm_fill_ghosts first — one fill per step saved when steps follow each other.  (A slab returns
 *      with its ghost PLANES exchanged and valid, and expects them so on entry.)  In LSM_MODE_FAST without a hook, when both
 *      faces of dimension 1 copy one node (periodic, symmetry, degree-0 extrapolation = NeumannBC), the stage kernels of
 *      these calls resolve the ghosts of dimension 1 in their loads and the fills inside the step leave the row ends alone
 *      (likewise dimension 2 of a 3-D grid): do not read those ghost nodes afterwards without an lsm_fill_ghosts of your own.
 *      hook may be NULL (the reference's default no-op update_func, src/levelsetterms.jl:63).
 *      On a slab handle with a communicator attached these run the slab's step (see "multi-GPU" below). */
int lsm_advance_fe(LsmHandle* h, const LsmTerm* terms, int nterms, void* phi, void* buf1,
                   double tc, double dt, LsmStageHook hook, void* user);
int lsm_advance_rk2(LsmHandle* h, const LsmTerm* terms, int nterms, void* phi, void* buf1, void* buf2,
                    double tc, double dt, LsmStageHook hook, void* user);
int lsm_advance_rk3(LsmHandle* h, const LsmTerm* terms, int nterms, void* phi, void* buf1, void* buf2,
                    double tc, double dt, LsmStageHook hook, void* user);

/* ---- SemiImplicitI2OE (src/timestepping.jl:204-426): ONE step of the semi-implicit I2OE scheme for a single AdvectionTerm,
 *      phi := A⁻¹ rhs with the reference's global system (:254-362; fac = dt/(2·Πh), inflow implicit, outflow explicit, face
 *      velocity ½(v_p + v_q) or v_p at a LinearExtrapolationBC ghost).  The velocity is term->coeff at time tc (CONST, ROTATION,
 *      SEPARABLE, FIELD); term->scheme is ignored, as in the reference.  The reference solves with a sparse direct solver; this
 *      call runs unpreconditioned BiCGSTAB, matrix-free, from x₀ = ϕ until ‖r‖₂ ≤ rtol·‖rhs‖₂ (the recursive residual), at most
 *      max_iters iterations, with every scalar on the device and the host reading the solver's status once per chunk of
 *      iterations.  Results therefore match the reference to the tolerance, not bitwise, and both arithmetic modes run the same
 *      solver.  Float32 storage: fp64 arithmetic throughout, the result rounded on store (LSM_DTYPE_F32).
 *      iters_out / rel_residual_out (may be NULL): iterations taken and ‖r‖₂/‖rhs‖₂.  Synchronous.
 *      LSM_ERR_INVALID (nothing runs): a term other than LSM_TERM_ADVECTION, fewer than 3 nodes in a dimension, a boundary
 *      condition other than periodic, NeumannBC (ExtrapolationBC degree 0) or LinearExtrapolationBC (degree 1), a communicator
 *      attached (single device only).  LSM_ERR_NOT_CONVERGED: breakdown (ρ, ω or r̂·v zero, or a non-finite value) or max_iters
 *      reached; lsm_last_error gives the iterations and the residual, and phi is left unchanged.
 *      The solver's device buffers (9 vectors + the face coefficients, ≈ 12 doubles per node in 3-D) are kept on the handle,
 *      grown on first use and freed by lsm_destroy. */
int lsm_advance_i2oe(LsmHandle* h, const LsmTerm* term, void* phi, double tc, double dt, double rtol, int max_iters, int* iters_out,
                     double* rel_residual_out);

/* ---- SemiLagrangian (not in the reference): ONE out-of-place step of a single AdvectionTerm by backward
 *      characteristics.  Every node I is traced back for dt in index space — trace 1: ξ = W(i − (dt·u(node, tc))/h); trace 2, the
 *      midpoint rule: ξᵐ = W(i − (½dt·u(node, tc + ½dt))/h), ξ = W(i − (dt·u(ξᵐ, tc + ½dt))/h) — and out[I] is the tensor-product
 *      Lagrange interpolant of phi at ξ on the centred stencil of 2, 4 or 6 nodes per dimension (order 1, 3, 5), clamped to the
 *      extrema of the departure cell's 2^N corners when limiter != 0 (Bermejo–Staniforth).  W wraps on an axis that is periodic
 *      (period n − 1) and clamps to [0, n − 1] on every other axis: a departure point outside the box reads the boundary.  The
 *      velocity is term->coeff (CONST, ROTATION, SEPARABLE, FIELD — interpolated linearly off the nodes, FIELD as it stands at the
 *      call); term->scheme is ignored.  A NaN velocity gives a NaN node and never an index outside the cell range.
 *      phi's ghost layers are filled on entry (all dimensions); the interior of out is written, its ghosts are STALE afterwards.
 *      Float32 storage: fp64 arithmetic, rounded once on store; both arithmetic modes run the same code and give the same bits.
 *      stats (may be NULL: the kernels then count nothing; a non-NULL pointer adds one record per workgroup, a small reduction
 *      behind the launch and a host wait): [0] workgroups that interpolated from the staged tile, [1] workgroups that read global
 *      memory, [2] the largest |dt·u_d/h_d| of the final trace over the grid — the displacement before W, since |ξ − i| means
 *      nothing across a wrap — in cells, rounded up (INT64_MAX for an infinite velocity).
 *      LSM_ERR_INVALID (nothing runs, nothing is written): out == phi or a null pointer; a term other than LSM_TERM_ADVECTION;
 *      order not 1, 3 or 5; trace not 1 or 2; dt negative or not finite; fewer than 2 nodes in a dimension; a slab handle or one
 *      with a communicator; an axis periodic on one face only.  With LSM_SEMILAG_STAGE = 2 also when a workgroup's departure box
 *      does not fit the staged tile (phi's ghosts are filled, out is untouched). */
int lsm_advance_semilag(LsmHandle* h, const LsmTerm* term, void* phi, void* out, double tc, double dt, int order, int trace, int limiter,
                        int64_t* stats);

/* ---- multi-GPU: the grid is cut into slabs of the LAST dimension, one handle per slab (lsm_create with an
 *      LsmSlab and LSM_BC_NONE on the faces towards neighbouring ranks — on BOTH faces of every rank when that dimension
 *      is periodic: the ring closes across the wrap, whose period is n-1, src/boundaryconditions.jl:107-119).  After every
 *      stage the LSM_GHOST full padded planes next to each interface are exchanged with rank±1 (they carry their own ghosts of
 *      the leading dimensions, so the corner composition of _getindexbc, src/meshfield.jl:248-260, is preserved), and Δt of
 *      compute_cfl is min-reduced over the ranks with NaN winning (src/levelsetterms.jl:22-28: `min` propagates NaN).
 *      Two transports:
 *        RCCL   one process per GPU.  Rank 0 calls lsm_comm_unique_id and hands the LSM_COMM_ID_BYTES to every rank out of
 *               band (MPI, a file, torch.distributed's store ...); then every rank calls lsm_comm_attach_rccl (collective).
 *               librccl is opened at run time; the planes travel as grouped ncclSend/ncclRecv over xGMI on a stream of the
 *               communicator's own, so that a stage's interior update overlaps the exchange of its boundary planes.
 *        LOCAL  all ranks are handles of ONE process (any devices): lsm_comm_attach_local(handles, world), one call.
 *               Planes move by peer copies.  lsm_halo_wait / lsm_allreduce_dt / lsm_advance_* block the calling thread until
 *               every rank of the group has made the matching call: drive the ranks from one host thread each, or from one
 *               thread stage by stage (lsm_stage_planes ..., lsm_halo_start on every handle, then lsm_halo_wait on every
 *               handle; reduce Δt yourself).
 *      With a communicator attached to a slab handle, lsm_advance_fe/rk2/rk3 run the slab's stages with the exchange
 *      overlapped (boundary planes first, interior while they travel) and expect phi's ghosts — boundary conditions and
 *      neighbour planes — valid on entry (they are on return; after writing the field from outside call
 *      lsm_fill_ghosts(h, phi, 7, NULL) + lsm_halo_exchange(h, phi)).  lsm_compute_cfl stays local: follow it with
 *      lsm_allreduce_dt.  lsm_destroy detaches. */
#define LSM_COMM_ID_BYTES 128
enum { LSM_COMM_NONE = 0, LSM_COMM_RCCL = 1, LSM_COMM_LOCAL = 2 };
int lsm_comm_unique_id(void* id_out /* LSM_COMM_ID_BYTES */);
int lsm_comm_attach_rccl(LsmHandle* h, const void* unique_id, int rank, int world);
int lsm_comm_attach_local(LsmHandle* const* handles, int world);     /* handles[r] = rank r */
int lsm_comm_detach(LsmHandle* h);
int lsm_comm_info(const LsmHandle* h, int* rank, int* world, int* transport);   /* any pointer may be NULL */
/* boundary-first stages with the exchange overlapped behind the interior update (default; LSM_SLAB_OVERLAP=0 in the
 * environment at attach time, or enable = 0, selects the plain stage -> ghost fill -> exchange order: same results) */
int lsm_comm_set_overlap(LsmHandle* h, int enable);
/* exchange of `field`'s ghost planes: start after the planes next to the interfaces are final on the handle's stream, wait
 * before anything reads the ghost planes (the handle's stream waits; no host synchronisation with RCCL) */
int lsm_halo_start(LsmHandle* h, void* field);
int lsm_halo_wait(LsmHandle* h);
int lsm_halo_exchange(LsmHandle* h, void* field);                    /* start + wait */
int lsm_allreduce_dt(LsmHandle* h, double* dt /* in: local, out: global */);   /* synchronous */
/* Failure: no call above blocks for ever.  When a rank leaves its group (lsm_comm_detach / lsm_destroy), calls lsm_comm_abort,
 * or does not show up within LSM_COMM_TIMEOUT_MS (environment, default 60000), every unfinished wait of the other ranks —
 * lsm_halo_wait, lsm_allreduce_dt, the slab lsm_advance_* — returns LSM_ERR_COMM, and so does every later call on that
 * communicator.  lsm_comm_abort may be called from any thread (e.g. by the rank whose update hook threw). */
int lsm_comm_abort(LsmHandle* h);

/* Slab-decomposed NarrowBandMeshField (BASELINE config 5's decomposition).  The band's operations reach farther across a slab
 * interface than a stencil does (nearest band node within 6 nodes, its slope neighbour, the stencil's 3:
 * src/meshfield.jl:481-530), so every rank creates its slab `overlap` planes larger towards each neighbouring rank (>= 10;
 * LsmSlab.lo / n describe the EXTENDED slab); the extra planes are ordinary planes of the slab, computed redundantly — right
 * on the owned planes — and refreshed from their owners:
 *   lsm_band_overlap_config  declares the overlap depth (after attaching the communicator)
 *   lsm_band_overlap_mask    after every lsm_band_update: the overlap planes of the byte mask from their owners (whole planes),
 *                            after which both sides list the band nodes of the exchanged planes in index order (no index
 *                            travels).  Synchronous.  Follow with lsm_band_overlap_values(vals), lsm_band_retile,
 *                            lsm_band_status, lsm_band_halo.
 *   lsm_band_overlap_values  after every stage (lsm_advance_band_* does it itself): the values of those band nodes, packed —
 *                            ~0.4 MB instead of 48 MB per direction at 768^3.  The handle's stream waits; no host sync with RCCL. */
int lsm_band_overlap_config(LsmHandle* h, int64_t overlap);
int lsm_band_overlap_mask(LsmHandle* h, void* mask);
int lsm_band_overlap_values(LsmHandle* h, void* field);

/* ---- EikonalReinitializationTerm(ϕ₀) constructor map: S0 = v/sqrt(v^2+Δx^2) (src/levelsetterms.jl:217-221) */
int lsm_eikonal_sign(LsmHandle* h, const void* phi0, void* s0_out, void* stream);

/* ---- min/max of the interior, for show (src/meshfield.jl:300-303) ---- */
int lsm_extrema(LsmHandle* h, const void* phi, double* vmin, double* vmax);
/* ---- is `phi` inside the domain of the handle's arithmetic mode?  *ok := 1 for LSM_MODE_STRICT handles and for fields
 *      with max|phi| <= LSM_FAST_MAX_ABS (NaN entries do not count: they propagate in both modes), else 0;
 *      *max_abs := max|phi| over the non-NaN interior values (may be NULL).  One reduction pass; synchronous. */
int lsm_check_range(LsmHandle* h, const void* phi, int* ok, double* max_abs);

/* ---- volume(ϕ) = prod(h)·Σ H(-ϕ) and perimeter(ϕ) = prod(h)·Σ δ(ϕ)‖∇ϕ‖ with the smoothed Heaviside /
 *      Dirac delta of width min(h) (src/levelsetops.jl:27-33,139-149,171-183) over the local slab;
 *      the usual posthook diagnostics.  lsm_perimeter refills phi's ghost layers (centred gradient).
 *      Synchronous. */
int lsm_volume(LsmHandle* h, const void* phi, double* out);
int lsm_perimeter(LsmHandle* h, void* phi, double* out);
/* ---- the same measures of a NarrowBandMeshField (src/levelsetops.jl:34-116,150-166), from the band alone.
 *      lsm_band_volume: prod(h)·(Σ_band H(-ϕ) + the number of off-band nodes inside): per grid line along dimension 1 the
 *      tails and the gaps between consecutive band nodes count when their end nodes are negative; a line without a band
 *      node takes the sign of the band node nearest (in index space) to its point n₁÷2, as the reference's KD-tree query
 *      does.  0 for an empty band.
 *      lsm_band_perimeter: the dense sum over the band nodes (the delta's support lies inside the band); phi must be a
 *      prepared stage input (lsm_band_prepare: the off-band neighbours of band nodes hold the extrapolated values).
 *      Single device; synchronous. */
int lsm_band_volume(LsmHandle* h, const void* phi, const void* mask, double* out);
int lsm_band_perimeter(LsmHandle* h, const void* phi, const void* mask, double* out);

/* ---- extend_along_normals!(F, ϕ; nb_iters, cfl, frozen, interface_band, min_norm)
 *      (src/velocityextension.jl:20-67): extends the speed F off the interface of ϕ by nb_iters
 *      first-order upwind sweeps of ∂τF + sign(ϕ) n·∇F = 0, frozen nodes held fixed.  F, phi and the
 *      work buffers (ndim+1 of them) are padded device arrays; frozen is NULL (band rule
 *      |ϕ| <= interface_band·Δ) or a padded array whose non-zero entries are frozen nodes.
 *      Ghosts of F are resolved with the handle's boundary conditions, as the reference does. */
int lsm_extend_along_normals(LsmHandle* h, void* F, void* phi, const void* frozen, void* work0, void* work1,
                             void* work2, void* work3, int nb_iters, double cfl, double interface_band,
                             double min_norm);

/* ---- curvature(ϕ, I), gradient(ϕ, I), normal(ϕ, I) (src/levelsetops.jl:197-226) at every node of the local slab,
 *      written to fp64 side arrays in the padded layout (out0 for the curvature, out0..out[ndim-1] for the vectors).
 *      phi's ghost layers are refilled on entry (centred differences reach one layer, corners included).
 *      The result is multiplied by `scale`.  band_width >= 0 evaluates only the nodes with |ϕ| <= band_width; the
 *      others get `fill`, and frozen_out (may be NULL; fp64 side array) := 1.0 on the evaluated nodes, 0.0 elsewhere —
 *      the seed-and-freeze loop of the reference's speed update functions (test/test-velocityextension.jl:118-131:
 *      v[I] = -curvature(ϕ, I) where |ϕ[I]| <= 1.5Δ, frozen there) in one launch, ready for
 *      lsm_extend_along_normals.  band_width < 0: every node.  Asynchronous on `stream` (NULL = the handle's). */
enum { LSM_GEOM_CURVATURE = 0, LSM_GEOM_GRADIENT = 1, LSM_GEOM_NORMAL = 2 };
int lsm_geometry(LsmHandle* h, int what, void* phi, double scale, double band_width, double fill, void* out0,
                 void* out1, void* out2, void* frozen_out, void* stream);
/*      The same at the active nodes of a NarrowBandMeshField (the reference's queries work on both field types,
 *      docs/src/geometry-queries.md): phi must be a prepared stage input (lsm_band_prepare: off-band neighbours hold the
 *      extrapolated values, out-of-grid ones the boundary values); nodes off the band get `fill` (frozen_out 0). */
int lsm_band_geometry(LsmHandle* h, int what, const void* phi, const void* mask, double scale, double band_width, double fill,
                      void* out0, void* out1, void* out2, void* frozen_out, void* stream);

/* ---- InterpolatedField(ϕ, order)(x) (src/interpolation.jl:117-151,228-260): value, gradient and Hessian of the piecewise
 *      polynomial interpolant of ϕ (Bernstein patch of the cell that holds x, odd orders interpolate, even orders fit
 *      a stencil one node larger; the interpolant `reinitialize!` measures distances to) at `npoints` points.
 *      points: npoints x ndim doubles on the device (point-major); values: npoints; gradients: npoints x ndim or NULL;
 *      hessians: npoints x ndim x ndim (row-major) or NULL.  order in 1..5.  phi's ghost layers are refilled on entry
 *      (dense fields; single device).  Asynchronous on `stream` (NULL = the handle's). */
int lsm_interpolate(LsmHandle* h, void* phi, int order, int64_t npoints, const void* points, void* values, void* gradients,
                    void* hessians, void* stream);

/* ---- NewtonSDF(ϕ; order, upsample, maxiters, xtol, ftol) (src/sdf.jl:57-127): the interface of a private copy of ϕ
 *      sampled once (the first half of reinitialize!), then signed distances at arbitrary points: exact nearest sample,
 *      Newton–Lagrange closest point on the seed cell's patch (further near samples as fall-back seeds),
 *      sign(dot(x - cp, ∇p(cp)))·‖x - cp‖.  phi: ghosts filled (dense) or a prepared band stage input with its mask.
 *      lsm_sdf_eval: points npoints x ndim doubles on the device; distances npoints; closest_points npoints x ndim or NULL;
 *      *nfail := queries whose solve did not converge (their best iterate is returned); NaN where the field has no
 *      interface sample at all.  lsm_sdf_samples: the nsamples x ndim sample points (get_sample_points).  Synchronous. */
typedef struct LsmSdf LsmSdf;
int lsm_sdf_create(LsmHandle* h, void* phi, const void* mask, int order, int upsample, int maxiters, double xtol, double ftol,
                   LsmSdf** out, int64_t* nsamples);
int lsm_sdf_eval(LsmSdf* s, int64_t npoints, const void* points, void* distances, void* closest_points, int64_t* nfail);
int lsm_sdf_samples(LsmSdf* s, void* points_out);
void lsm_sdf_destroy(LsmSdf* s);

/* ---- quadrature(ϕ; interpolation_order, quadrature_order, surface) (src/LevelSetMethods.jl:103-126,
 *      ext/ImplicitIntegrationExt.jl): nodes and weights integrating over {ψ < 0} (surface = 0) or {ψ = 0} (surface = 1) of
 *      the piecewise interpolant ψ of degree interpolation_order (1..5), quadrature_order (1..20) Gauss–Legendre points per
 *      direction, by R. Saye's algorithm on every cell's Bernstein patch.  phi: a dense field (its ghost
 *      layers are refilled on entry; mask NULL) or a prepared band stage input with its mask (surface only; the band's
 *      active cells).  Single device.  Cells are linear indices over the (n-1)^N cells, axis 0 fastest, ascending.
 *      lsm_quad_create: counts[4] := {cut cells with nodes, nodes, full cells, boxes that reached the depth limit}.
 *      lsm_quad_read copies into device buffers (each may be NULL): cells ncut int64; offsets ncut+1 int64 (the nodes of
 *      cut cell i are offsets[i]..offsets[i+1]-1); coords nodes x ndim doubles (point-major); weights nodes doubles;
 *      full_cells nfull int64 (volume: cells whose coefficients are all < 0; their rule is the tensor rule mapped to the
 *      cell); rule_coords q^ndim x ndim and rule_weights q^ndim doubles, that rule on the unit cell.  lsm_quad_total: the
 *      sum of every weight, full cells included.  Synchronous. */
typedef struct LsmQuad LsmQuad;
int lsm_quad_create(LsmHandle* h, void* phi, const void* mask, int interpolation_order, int quadrature_order, int surface,
                    LsmQuad** out, int64_t* counts);
int lsm_quad_read(LsmQuad* s, void* cells, void* offsets, void* coords, void* weights, void* full_cells, void* rule_coords,
                  void* rule_weights);
int lsm_quad_total(LsmQuad* s, double* total);
void lsm_quad_destroy(LsmQuad* s);

/* ---- isosurface(ϕ, level): the interface {ϕ = level} as an indexed mesh — what export_surface_mesh gets from marching
 *      cubes over values(ϕ) (ext/MMGSurfaceExt.jl:48-50) and what ext/MakieExt.jl draws (contour!(…; levels = [0]) in
 *      2-D, an iso-volume in 3-D).  Marching simplices on the Freudenthal subdivision of every cell (2 triangles in 2-D,
 *      6 tetrahedra in 3-D): a watertight, consistently oriented mesh of the zero set of the
 *      piecewise-linear interpolant with shared vertices; normals point from ϕ < level to ϕ >= level.  phi: a dense field
 *      (mask NULL) or a band field with its mask (the cells whose corners are all band nodes); only the interior is read:
 *      no ghost fill, stale ghosts do not matter.  2-D and 3-D, single device, level finite; an empty result is LSM_OK.
 *      lsm_iso_create: counts[2] := {vertices, elements}.  lsm_iso_read copies into device buffers (each may be NULL):
 *      vertices nv x ndim doubles (point-major), ordered by the grid node that owns the vertex's edge (axis 0 fastest);
 *      elements ne x ndim int64, 0-based vertex numbers (segments in 2-D, triangles in 3-D), ordered by cell.
 *      Synchronous. */
typedef struct LsmIso LsmIso;
int lsm_iso_create(LsmHandle* h, const void* phi, const void* mask, double level, LsmIso** out, int64_t* counts);
int lsm_iso_read(LsmIso* s, void* vertices, void* elements);
void lsm_iso_destroy(LsmIso* s);

/* ---- mesh_distance(mesh, grid, cutoff): from a mesh back to a level set — the inverse of lsm_iso_*.  phi_out[I] :=
 *      s(I)·min(d(I), cutoff) over the interior of a dense field of the handle (the ghosts are left as they are: fill them
 *      before a stencil reads them): d the exact Euclidean distance from node I to the nearest element, s = −1 where the mesh
 *      winds around the node and +1 elsewhere (tests/_mdist_ref.py restates every operation).  vertices:
 *      nverts x ndim doubles (point-major), elements: nelems x ndim int64, 0-based vertex numbers (segments in 2-D, triangles
 *      in 3-D), both device buffers, oriented as lsm_iso_*'s (normals pointing out of the region that becomes phi < 0); the
 *      mesh must be closed and consistently oriented.  0 < cutoff <= +inf: the work is the sum of the elements' bounding
 *      boxes dilated by the cutoff, so a finite cutoff of a few cells is what a narrow band or a reinitialisation needs; nodes
 *      beyond it carry ±sqrt(cutoff·cutoff).  All arithmetic is fp64; an f32 handle rounds on store.  The sign is a crossing
 *      count along axis 0 with a half-open inclusion rule (a grid line through a shared edge or vertex is counted once); the
 *      result is deterministic bit for bit.  stats[3] (may be NULL) := {nodes with d < cutoff, grid rows whose crossings do
 *      not balance — non-zero: the mesh is open or inconsistently oriented and the signs along those rows mean nothing —,
 *      elements skipped by the sign pass because their projection along axis 0 is degenerate}.  LSM_ERR_INVALID: a slab
 *      handle, a 1-D grid, cutoff <= 0 or NaN, a vertex number outside 0..nverts-1 (checked on the device before anything is
 *      addressed with it), a non-finite vertex.  An empty mesh is LSM_OK: phi_out = +sqrt(cutoff·cutoff).  stream: NULL = the
 *      handle's.  The scratch arrays (8 bytes per node, 4 bytes per node and row) belong to the handle and only grow.
 *      Synchronous. */
int lsm_mesh_distance(LsmHandle* h, int64_t nverts, const void* vertices, int64_t nelems, const void* elements, double cutoff,
                      void* phi_out, int64_t stats[3], void* stream);

/* ---- eikonal_(phi, speed, width, cutoff): |grad T| = s = 1/F on the dense grid, first-order Godunov upwind, solved by the
 *      block-based fast iterative method (csrc/lsm_eikonal.hip; tests/_eikonal_ref.py restates every
 *      operation).  phi[I] := copysign(min(T[I], cutoff), phi[I]) over the interior of a dense field of the handle (the ghosts
 *      are left as they are: fill them before a stencil reads them).  speed NULL: s = 1, T is the distance to the interface —
 *      a far-field redistancing in O(nodes); otherwise a device array of one double per interior node, n-shaped, axis 0
 *      fastest (no ghosts), and T is the travel time of a front of speed F.  Inside and outside are solved as one
 *      non-negative T.  A node is frozen (T given) or free (T starts at +inf); neighbours off the grid do not exist, whatever
 *      the boundary condition.
 *      The update G of a free node I: a_d = min(T[I-e_d], T[I+e_d]) over the neighbours that exist; the axes with a_d = +inf
 *      are dropped (none left: G = +inf); the rest sorted by (a_d, d); a0 the smallest, tau = s_I·h of its axis; for k = 2, 3:
 *      stop unless a0 + tau > a_k; over the first k axes, w_d = 1/(h_d·h_d), delta_d = a_d - a0, A = sum w, B = sum w·delta,
 *      C = sum (w·delta)·delta - s_I·s_I, disc = B·B - A·C, stop if disc < 0, tau = (B + sqrt(disc))/A; G = a0 + tau.  I takes
 *      T := G only when G < T.  (The quadratic is solved for T - a0: the un-shifted form cancels like (a/h)^2.)
 *      Seeding: phi_I = 0 is frozen at T = 0.  I is crossing-adjacent when phi_I != 0 and an axis neighbour J that exists has
 *      (phi_J > 0) != (phi_I > 0) or phi_J = 0.  width = 0 (the crossing seed, any phi): per axis sigma_d = min over such J of
 *      h_d·(|phi_I|/(|phi_I| + |phi_J|)), T_I = s_I/sqrt(sum_d 1/(sigma_d·sigma_d)) over the axes with a crossing; every other
 *      node is free.  width = w > 0 (phi already holds distances or times near the interface: after lsm_reinitialize, after
 *      lsm_mesh_distance with a cutoff > w): every node with |phi_I| <= w and every crossing-adjacent node is frozen at
 *      T_I = |phi_I|.
 *      0 < cutoff <= +inf: nodes with T <= cutoff hold the values they hold without a cutoff, the others ±cutoff; the front
 *      is not followed beyond it.  max_iters: the bound on the outer iterations (launches of the tile kernel); <= 0: 2·sum_d n_d.
 *      stats[4] (may be NULL) := {frozen nodes, outer iterations, tile visits, nodes clamped at the cutoff}.
 *      LSM_ERR_INVALID without running anything: a 1-D grid, a handle with a communicator or of a slab, a periodic dimension,
 *      fewer than two nodes in a dimension, width < 0 or not finite, cutoff <= 0 or NaN.  (There is no mask parameter: the
 *      values array of a band field is not a dense field, and the caller must not pass one.)  LSM_ERR_INVALID after the seed
 *      kernel, which only reads phi: a non-finite phi (reason 1), a speed that is not finite and positive (2), no frozen node at
 *      all: phi has no interface (3); stats := {-reason, offending nodes, 0, 0} then, and stats[0] >= 0 in every other return.  LSM_ERR_NOT_CONVERGED: the active list was not empty after max_iters outer iterations.  In every
 *      failure phi is untouched: only the final pass writes it.  All arithmetic is fp64; an f32 handle is read once and
 *      rounded once on store.  Neighbouring tiles run concurrently; T only decreases, so the fixed point does not depend on
 *      the schedule beyond rounding (tests/test_gpu_eikonal.py).  stream: NULL = the handle's.  The scratch arrays (9 bytes
 *      per node, 5 per tile) belong to the handle and only grow.  Synchronous. */
int lsm_eikonal(LsmHandle* h, void* phi, const double* speed, double width, double cutoff, int64_t max_iters, int64_t stats[4],
                void* stream);

/* ---- extend_from_interface_(F, phi): K <= 8 fields carried off a frozen set along the characteristics of |phi|,
 *      grad F · grad |phi| = 0, first-order upwind, each value computed exactly once on lsm_eikonal's tile lists
 *      (csrc/lsm_eikonal.hip; tests/_extend_ref.py restates every operation).  This comment is the rule.
 *      phi: a dense field of the handle, read only (interior only).  F[0..nfields): fields of the handle in phi's padded layout
 *      and storage type (device pointers; the array F itself is on the host), updated in place over the interior, the ghosts
 *      left as they are.  Neighbours off the grid do not exist, whatever the boundary condition.  The key of node I is
 *      g_I = |phi_I|, except under LSM_EXTEND_INSIDE, g_I = phi_I, and LSM_EXTEND_OUTSIDE, g_I = -phi_I: the same at the free
 *      nodes, but with every frozen node below every free one (with |phi| a free node next to the interface whose frozen
 *      neighbour sits deeper than it sits itself would have nobody to take a value from); w_d = 1/(h_d·h_d).
 *      The frozen set.  LSM_EXTEND_RULE: lsm_eikonal's seeding set — I is crossing-adjacent when phi_I != 0 and an axis
 *      neighbour J that exists has (phi_J > 0) != (phi_I > 0) or phi_J = 0; width = 0: the crossing-adjacent nodes and the
 *      nodes with phi_I = 0; width = w > 0: the crossing-adjacent nodes and every node with |phi_I| <= w.  LSM_EXTEND_MASK:
 *      `frozen`, a device array of one byte per interior node, n-shaped, axis 0 fastest; non-zero: frozen.
 *      LSM_EXTEND_INSIDE: phi_I <= 0.  LSM_EXTEND_OUTSIDE: phi_I >= 0.  `frozen` is read by LSM_EXTEND_MASK only.
 *      The seeds.  LSM_EXTEND_NODES: a frozen node keeps its F.  LSM_EXTEND_INTERFACE (with LSM_EXTEND_RULE only): a
 *      crossing-adjacent node I takes the value at its crossings, computed from the input fields: per axis d with a crossing,
 *      among the crossing neighbours the J with the smaller sigma_d = h_d·theta, theta = |phi_I|/(|phi_I| + |phi_J|) (a tie:
 *      the - side); Fc_d = F_I + theta·(F_J - F_I), u_d = 1/(sigma_d·sigma_d); F_I := (sum_d u_d·Fc_d)/(sum_d u_d), the axes
 *      ascending, the sums started at 0, clamped to [min_d Fc_d, max_d Fc_d] (below).  Every other frozen node keeps its F.
 *      A node that is not frozen and has |phi_I| >= cutoff (0 < cutoff <= +inf) takes `fill` (counted in stats[4]).
 *      Every other node is free.  Per axis d, a_d is the smaller key of its two axis neighbours (one, at a face), J_d the
 *      neighbour that holds it (a tie: the - side).  Axis d participates iff a_d < g_I, strictly; c_d = w_d·(g_I - a_d).
 *      F_I = (sum_d c_d·F_Jd)/(sum_d c_d) over the participating axes, ascending, the sums started at 0, plain multiplies and
 *      adds (no fused multiply-add); then the clamp: r = the quotient; if not r >= lo then r = lo; if not r <= hi then r = hi,
 *      with lo and hi the smallest and the largest F_Jd of the participating axes.  The clamp changes the quotient by
 *      rounding at most; with it every value lies within the minimum and the maximum of the seeds exactly and a constant comes
 *      back as it is.  A free node with no participating axis is an orphan: it keeps its input value and behaves as a frozen
 *      node in every respect (counted in stats[3]); orphans appear where phi is not distance-like and on ties of rounded
 *      values; the plateau beyond lsm_eikonal's cutoff is filled, not orphaned, when the same cutoff is passed.  The
 *      dependencies are acyclic by the strict inequality, so every free node is reached whatever phi holds, every value is
 *      computed once from final values, and the result does not depend on the tile schedule: the same bits in every run.
 *      Refused with LSM_ERR_INVALID after one pointwise kernel, before any field is written: a non-finite phi (reason 1), a
 *      non-finite F_k at a frozen node or an orphan (2), no frozen node at all (3); stats := {-reason, offending nodes, 0, 0, 0}
 *      then.  The input values at the other nodes are never read and may be NaN.
 *      max_iters: the bound on the outer iterations (rebuilds of the tile list, each followed by one launch of the tile
 *      kernel over the listed tiles and all fields); <= 0: 2·sum_d n_d.  LSM_ERR_NOT_CONVERGED: the list was not empty after
 *      max_iters iterations, or — an internal error, the message says so — it emptied with values left uncomputed.
 *      stats[5] (may be NULL) := {frozen nodes by the rule or the mask, outer iterations, tile visits, orphans, filled nodes}.
 *      LSM_ERR_INVALID without running anything: a 1-D grid, a handle with a communicator or of a slab, a periodic dimension,
 *      fewer than two nodes in a dimension, nfields outside 1…8, a null field, the same field twice, a field that is phi,
 *      width < 0 or not finite, cutoff <= 0 or NaN, a non-finite fill, LSM_EXTEND_MASK without a mask, an unknown rule or
 *      source, LSM_EXTEND_INTERFACE with another rule than LSM_EXTEND_RULE.  In every failure the fields are untouched: only
 *      the final pass writes them.  All arithmetic is fp64; an f32 handle is read once and rounded once on store.  stream:
 *      NULL = the handle's.  The scratch arrays are lsm_eikonal's and 8·nfields bytes per node; they belong to the handle and
 *      only grow.  Synchronous. */
enum { LSM_EXTEND_RULE = 0, LSM_EXTEND_MASK = 1, LSM_EXTEND_INSIDE = 2, LSM_EXTEND_OUTSIDE = 3 };
enum { LSM_EXTEND_NODES = 0, LSM_EXTEND_INTERFACE = 1 };
int lsm_extend(LsmHandle* h, const void* phi, void* const* F, int nfields, int frozen_rule, const unsigned char* frozen,
               double width, int source, double cutoff, double fill, int64_t max_iters, int64_t stats[5], void* stream);

/* ---- components(ϕ, level, side): the connected components of the set S = {ϕ < level} (side 0) or of its complement (side 1)
 *      on the dense grid, labelled on the device by block-based union–find (csrc/lsm_cc.hip, DESIGN.md §7.16;
 *      tests/_cc_ref.py restates the definition).  inside(I) := ϕ[I] < level, as lsm_iso_*: ϕ == level is outside.  Two nodes
 *      of S are adjacent iff they differ by ±d for some d in {0,1}^ndim \ {0}: the edges of the Freudenthal (Kuhn)
 *      subdivision that lsm_iso_* and lsm_vol_* cut — 6 neighbours in 2-D, 14 in 3-D, not the 4/8 or 6/26 neighbourhoods of
 *      image libraries — so the components of side 0 are exactly the vertex-connected pieces of lsm_vol_*'s mesh.  Components
 *      are numbered 0 … K−1 in ascending order of their smallest linear node index (axis 0 fastest); the result does not
 *      depend on the schedule.  Only the interior of phi is read.
 *      lsm_cc_create: stats[4] (may be NULL) := {K, nodes in S, Kuhn edges between two nodes of S in different tiles (8x8x8;
 *      32x8 in 2-D), non-finite nodes}.  LSM_ERR_INVALID: a 1-D grid, a slab handle or one with a communicator, a periodic
 *      dimension (the wrap would join components), level not finite, side not 0 or 1, 2^31 − 1 nodes or more, a non-finite
 *      phi (stats[3] > 0; stats is filled).  (There is no mask parameter: the values array of a band field is not a dense
 *      field, and the caller must not pass one.)  An empty S is LSM_OK with K = 0.
 *      lsm_cc_read copies into device buffers (each may be NULL): labels, one int32 per interior node, n-shaped, axis 0
 *      fastest, −1 off S; nodes int64[K]; index_sums int64[K][ndim], the sums of the 0-based node indices per axis;
 *      bbox int32[K][2][ndim], the smallest and the largest index per axis.  All are integers: exact, whatever the order of
 *      the additions.
 *      lsm_cc_flip moves every node of the components k with which[k] != 0 (K bytes on the device) to the other side of
 *      level, in place: v' = level + (level − v), two fp64 operations without contraction; for side 1, where v' is not
 *      < level it becomes the double just below level; f32 storage is read widened, rounded once, and where the rounded
 *      value is on the wrong side it is replaced by the neighbouring float on the right side.  *flipped := the number of
 *      nodes written.  A first pass counts the flagged nodes that the current phi does not put on the object's side; when
 *      there is one the call fails with LSM_ERR_INVALID and phi is untouched (phi changed since lsm_cc_create, or the
 *      components were flipped already).  The ghosts are left as they are, and the result is no distance function near what
 *      was removed.  The parent array (4 bytes per node) belongs to the handle and only grows; the labels (4 bytes per node)
 *      and the statistics belong to the object.  Synchronous, on the handle's stream. */
typedef struct LsmCc LsmCc;
int lsm_cc_create(LsmHandle* h, const void* phi, double level, int side, LsmCc** out, int64_t stats[4]);
int lsm_cc_read(LsmCc* s, void* labels, void* nodes, void* index_sums, void* bbox);
int lsm_cc_flip(LsmCc* s, void* phi, const void* which, int64_t* flipped);
void lsm_cc_destroy(LsmCc* s);

/* ---- nucleation: the centres that a criterion field t selects on phi's grid, and the punch that removes a ball around each — the
 *      step by which a level-set optimisation creates holes (csrc/lsm_nucleate.hip; tests/_topo_ref.py restates
 *      the definition).  t is any dense field of the handle: the topological derivative of lsm_elastic_topo, a criterion of the
 *      caller's, T − l with a volume multiplier.  Only the interiors of phi and t are read; values are converted to fp64 first.
 *      Candidates: the interior node I is a candidate iff t_I < threshold and phi_I <= level − clearance (the difference formed once,
 *      in fp64); both are false for NaN.  phi is taken to be roughly a signed distance, so that a candidate lies at least
 *      `clearance` inside the material: that is the caller's business.
 *      Centres: w_d = ceil(spacing/h_d) nodes per axis.  I is a centre iff it is a candidate and its key (t_I, linear index I, axis 0
 *      fastest) is the lexicographic minimum over the candidates J with |J_d − I_d| <= w_d for every d, the window clipped at the
 *      grid; −0 and +0 are one value.  Two centres differ by more than w_d nodes along some axis, hence lie more than `spacing`
 *      apart; the list does not depend on the schedule.
 *      lsm_nucleate_create: *count := the number of centres.  lsm_nucleate_read copies into device buffers (each may be NULL):
 *      indices int64[count], the linear indices in ascending order, and values fp64[count], t at them.  LSM_ERR_INVALID: a 1-D
 *      grid, a slab handle or one with a communicator, a periodic dimension (the window does not wrap), a non-finite threshold,
 *      level, clearance or spacing, a w_d outside [1, 32], 2^31 − 1 nodes or more.  No centre is LSM_OK with count 0.
 *      lsm_nucleate_punch, for `count` linear node indices on the device (any list: the centres above, a part of them, the caller's
 *      own; repeats allowed): B_d = floor(radius/h_d) in fp64, and for the node I of the box |I_d − c_d| <= B_d of centre c,
 *      clipped at the grid, d2 = sum_d ((I_d − c_d)·h_d)², d ascending from +0, the difference converted exactly; v = level +
 *      (radius − sqrt(d2)), no contraction.  V_I = the largest v over the centres whose box holds I; phi_I := V_I where phi_I < V_I
 *      (false for a NaN phi, which stays), rounded once to the storage type; every other node and the ghosts are untouched.  The
 *      maximum commutes, so the result does not depend on the order of the list or on the schedule.  *changed := the number of
 *      nodes whose stored bits changed.  With radius < h_d for every d only the centres themselves can change.  The result is the
 *      distance to the ball inside it and no distance function around it: reinitialize afterwards.  LSM_ERR_INVALID with phi
 *      untouched: the refusals of lsm_nucleate_create, a non-finite level, a radius not finite and positive, a negative count, an
 *      index outside the grid.  count == 0 is LSM_OK and runs nothing.
 *      The window keys (24 bytes per node) belong to the handle and only grow; the lists belong to the object.  Synchronous, on
 *      the handle's stream. */
typedef struct LsmNucleate LsmNucleate;
int lsm_nucleate_create(LsmHandle* h, const void* phi, const void* t, double threshold, double level, double clearance, double spacing,
                        LsmNucleate** out, int64_t* count);
int lsm_nucleate_read(LsmNucleate* s, void* indices, void* values);
void lsm_nucleate_destroy(LsmNucleate* s);
int lsm_nucleate_punch(LsmHandle* h, void* phi, const void* centres, int64_t count, double level, double radius, int64_t* changed);

/* ---- elliptic_solve: −∇·(a∇u) + c·u = f on the box of a dense 2-D or 3-D grid, the state equation of a shape optimisation with
 *      an ersatz material outside the level set, and with constant coefficients the H¹ regularisation (I − α²Δ)V = g; solved on
 *      the device by conjugate gradients preconditioned by one geometric multigrid V-cycle (csrc/lsm_elliptic.hip, DESIGN.md
 *      §7.17; tests/_elliptic_ref.py restates every operation).  Unknowns at the nodes; natural (zero-flux) conditions on every
 *      face; a caller-given set of fixed (Dirichlet) nodes.  Node arrays are n-shaped fp64 on the device, axis 0 fastest, no
 *      ghosts; the cell array has n−1 entries per axis.  All arithmetic is fp64, without contraction.
 *      Cell coefficient, for a cell with 2^N corners: mean = (sum of the corner values of phi in ascending linear index)·2^−N;
 *      theta = min(max(1/2 − (mean − level)/min_d h_d, 0), 1); a = a_out + (a_in − a_out)·theta.  Or a_cells != NULL: the cell
 *      array is the caller's (phi may be NULL then).
 *      Edge coefficient, along d between I and I+e_d: S = the sum of a over the existing cells that share the edge, in ascending
 *      linear index; k = S·2^−(N−1) (a boundary edge carries half or a quarter: the faces are natural); kbar = S/(number of
 *      those cells); w = k·ih2_d with ih2_d = 1/(h_d·h_d).  Node mass m_I = (existing cells around I)/2^N.
 *      Operator, scaled by 1/prod h: (A u)_I = sum_d [ w_minus·(u_I − u_{I−e_d}) + w_plus·(u_I − u_{I+e_d}) ] + (c_I·m_I)·u_I,
 *      accumulated from +0 in this order: d ascending, the minus side before the plus side, sides that do not exist skipped,
 *      the c term last.  The right-hand side is b_I = m_I·f_I.  A is symmetric.  c: c_nodes (n-shaped) or c_const.
 *      Fixed nodes (fixed: one byte per node, non-zero = fixed; NULL: none) keep u_I exactly; their rows and columns are
 *      eliminated: r0 = b − A u0 on the free nodes with u0 = u as passed (the Dirichlet values on the fixed nodes, the guess
 *      elsewhere); search directions are zero on fixed nodes.
 *      Solver: PCG on the free nodes until the recursive ||r||_2 <= rtol·||b_free||_2 (||r0||_2 where b_free is zero).  The
 *      scalars and the status live on the device; iterations are enqueued in chunks.  precond LSM_PRECOND_JACOBI: D^−1.
 *      LSM_PRECOND_MG: one V-cycle from zero.  Coarsening per dimension: axis d coarsens while n_d > 5, to (n_d+1)/2 nodes;
 *      coarse node J sits on fine node 2J and h_d doubles; an axis that stopped is carried unchanged; the hierarchy ends when
 *      no axis coarsens (the coarsest level has at most 5 nodes per axis).  For an even n_d the last fine node has no coarse
 *      partner.  Prolongation, a tensor product of: fine 2J <- J; fine 2J+1 <- (J + (J+1))/2, or J alone where J+1 does not
 *      exist.  Restriction = P^T/2^(coarsened axes); fine residuals are zero on fixed nodes; a coarse node is fixed iff fine
 *      node 2J is; corrections are zero on fixed nodes.  Coarse operator: the same discretisation with the coarse cell's a the
 *      arithmetic mean of the fine cells {2J, 2J+1} per coarsened axis, c injected.  Smoother: damped Jacobi, omega = 0.8,
 *      x <- x + omega·(r − A x)/D, 2 sweeps before and 2 after; the first sweep from zero is omega·r/D; the coarsest level
 *      runs 16 such sweeps from zero.
 *      lsm_elliptic_create builds the hierarchy (owned by the caller: lsm_elliptic_destroy frees it with its scratch, about
 *      10 doubles per node).  stats[4] (may be NULL) := {levels, free nodes, fixed nodes, 0}.  LSM_ERR_INVALID without running
 *      anything: a 1-D grid, a slab handle or one with a communicator, a periodic dimension, fewer than 3 nodes in a dimension,
 *      a_in / a_out not finite and positive, c_const negative or not finite, an unknown precond.  (There is no mask parameter:
 *      the values array of a band field is not a dense field, and the caller must not pass one.)  LSM_ERR_INVALID after the
 *      setup kernel, with stats := {−reason, offending entries, 0, 0}: a non-finite phi (1), a cell coefficient not finite and
 *      positive (2), a c not finite or negative (3), no fixed node and c = 0 everywhere: singular (4), every node fixed (5).
 *      lsm_elliptic_apply: y = A x on all nodes, no elimination (so that tests can see the operator).
 *      lsm_elliptic_solve: f n-shaped fp64; u a dense field of the handle: in, the guess and the Dirichlet values; out, the
 *      solution on the free nodes, rounded once to the storage type; fixed nodes and ghosts are left as they are.
 *      LSM_ERR_INVALID: a non-finite f or u.  LSM_ERR_NOT_CONVERGED: breakdown or max_iters.  In every failure u is untouched.
 *      *iters, *relres (may be NULL) := the iterations and the recursive ||r||/||b_free||.  stream: NULL = the handle's.
 *      lsm_elliptic_energy: e_I = sum_d ( sum over the sides that exist, minus first, of kbar·(g·g), g = (u_J − u_I)/h_d )
 *      / (number of existing edges along d at I), d ascending, into a dense field of the handle (rounded once).
 *      lsm_elliptic_compliance: *out := prod h · sum_I (m_I·f_I)·u_I, reduced on the device.
 *      lsm_elliptic_cells copies the level-0 cell array into a device buffer.  All but solve run on the handle's stream;
 *      solve, compliance and create are synchronous.
 *      lsm_elliptic_solve_many: K sources of the one operator (1 <= K <= LSM_ELLIPTIC_MAXCOLS) solved in the same launches.
 *      Column k of the batch is lsm_elliptic_solve of column k, bit for bit: the field, the iteration count and the relative
 *      residual (every column has the single solve's launch shape, arithmetic and order, and its own device state).  f is
 *      K·nn fp64 on the device, column k at k·nn; u[k] is the field of column k, K distinct dense fields of the handle holding
 *      the guess and the Dirichlet values.  iters, relres and status are host arrays of K, filled for every column whatever
 *      the outcome; status: 1 converged, 2 out of iterations, −1 non-finite input, −2 breakdown (p·Ap not positive), −3
 *      breakdown (r·Mr not positive, or a non-finite residual).  A column that has ended is skipped by its own workgroups while
 *      the others go on.  LSM_OK only when all columns converged, and only then are the free nodes of all columns stored;
 *      otherwise no field of any column changes, the converged ones included, and the error is LSM_ERR_INVALID if a column had
 *      non-finite input, else LSM_ERR_NOT_CONVERGED; the message names the lowest such column with its iterations and residual.
 *      LSM_ERR_INVALID without running anything: K out of range, a null or repeated field, rtol not positive and finite,
 *      max_iters < 1.  The batch has a workspace of its own (7 doubles per node and column on level 0, 3 on the others),
 *      allocated by the first call, kept on the object and grown when a later call asks for more columns; when it cannot be
 *      allocated the HIP error is returned and the object stays usable.  lsm_elliptic_solve and the modes of the object are
 *      unaffected by a batched call in between.  Not to be called concurrently with another call on the object.
 *      lsm_elliptic_energy_many: e_I = sum_k w_k·e_{k,I}, k ascending from +0, e_{k,I} lsm_elliptic_energy's value of column k
 *      in fp64 before its rounding; rounded once to the storage type, ghosts untouched; one pass over the grid.
 *      LSM_ERR_INVALID: K out of range, a null or repeated field, an output that is an input, a weight that is not finite.
 *      lsm_elliptic_energy_mutual: m_I = lsm_elliptic_energy's sums with g·g replaced by g_u·g_v, g_u = (u_J − u_I)/h_d and g_v the
 *      same for v, in the same order, rounded once: the integrand of the shape derivative of l·u for the state A u = f and
 *      the adjoint A v = l.  With v = u it is lsm_elliptic_energy bit for bit; m(u, v) and m(v, u) are the same bits.  Like
 *      lsm_elliptic_energy it is the a∇u·∇v part only: the c·u·v term is not in it.  u and v may be the same field;
 *      LSM_ERR_INVALID: a null field, an output that is an input. */
#define LSM_PRECOND_MG 0
#define LSM_PRECOND_JACOBI 1
typedef struct LsmElliptic LsmElliptic;
int lsm_elliptic_create(LsmHandle* h, const void* phi, double level, double a_in, double a_out, const double* a_cells, double c_const,
                        const double* c_nodes, const void* fixed, int precond, LsmElliptic** out, int64_t stats[4]);
int lsm_elliptic_apply(LsmElliptic* s, const double* x, double* y);
int lsm_elliptic_solve(LsmElliptic* s, const double* f, void* u, double rtol, int max_iters, int* iters, double* relres, void* stream);
int lsm_elliptic_energy(LsmElliptic* s, const void* u, void* e_out);
int lsm_elliptic_compliance(LsmElliptic* s, const double* f, const void* u, double* out);
int lsm_elliptic_cells(LsmElliptic* s, double* a_out_cells);
#define LSM_ELLIPTIC_MAXCOLS 8
int lsm_elliptic_solve_many(LsmElliptic* s, int K, const double* f, void* const* u, double rtol, int max_iters, int* iters, double* relres,
                            int* status, void* stream);
int lsm_elliptic_energy_many(LsmElliptic* s, int K, void* const* u, const double* w, void* e_out);
int lsm_elliptic_energy_mutual(LsmElliptic* s, const void* u, const void* v, void* e_out);
void lsm_elliptic_destroy(LsmElliptic* s);

/* ---- elasticity_solve: −∇·σ(u) = f on the box of a dense 2-D or 3-D grid, σ = E(x)·C0(ν):ε(u), the state equation of a
 *      structural (compliance) shape optimisation with an ersatz material outside the level set; Q1 elements, the N displacement
 *      components at the nodes, traction-free faces, a caller-given set of fixed displacement components; solved on the device by
 *      conjugate gradients preconditioned by one geometric multigrid V-cycle (csrc/lsm_elastic.hip, DESIGN.md §7.18;
 *      tests/_elastic_ref.py restates every operation).  Shapes, ownership, streams and failures are lsm_elliptic_*'s.
 *      Cell modulus: exactly lsm_elliptic's cell formula with (e_in, e_out) for (a_in, a_out) — the same code, the same bits —
 *      or e_cells != NULL: the caller's cell array (phi may be NULL then).
 *      Material at E = 1: mu = 1/(2(1+nu)); lambda = nu/((1+nu)(1−2nu)) in 3-D and for LSM_PLANE_STRAIN, lambda = nu/(1−nu²) for
 *      LSM_PLANE_STRESS (plane is ignored in 3-D, but must be one of the two).  nu finite with −1 < nu < 0.5.
 *      Unit element matrix of a level, for a box cell with sides h, scaled by 1/prod h as the scalar operator is:
 *        K0[(a,i),(b,j)] = (1/prod h)·∫_cell lambda·d_i N_a·d_j N_b + mu·d_j N_a·d_i N_b + delta_ij·mu·grad N_a·grad N_b,
 *      exact for the multilinear shape functions N_a; corner a has bit d set when it sits on the cell's upper side along d; the row
 *      index is a·N + i; (2^N·N)² doubles, row-major.  It is computed on the host in fp64, once per level (h doubles on the axes
 *      that coarsen): G[a,b,i,j] = ∫ d_i N_a d_j N_b is the product over the axes d, ascending from 1.0, of the 1-D factors
 *      stiffness ((a_d == b_d ? 1 : −1)/h_d: i == j == d), mixed (+1/2 when the differentiated corner has bit d set, else −1/2:
 *      i != j and d == i takes a's bit, d == j takes b's) and mass (h_d/3 when a_d == b_d, else h_d/6: every other axis);
 *      K0 = ((lambda·G[a,b,i,j] + mu·G[a,b,j,i]) + [i == j]·mu·(sum_k G[a,b,k,k], k ascending from 0))/(1·h_0·h_1·…).
 *      lsm_elastic_stiffness copies a level's K0, as the device holds it, into a host array.
 *      Unknowns: solver vectors are component-major fp64 on the device, x[i·nn + id], id = i0 + n0·(i1 + n1·i2), no ghosts.
 *      Operator: (A u)_{I,i} = sum over the cells C around I of E_C·(sum_b sum_j K0[(a,i),(b,j)]·u_{b,j}), a = I's corner in C.  The
 *      cells in ascending order m = 0 … 2^N−1 (bit d of m set: cell index I_d along d, clear: I_d − 1; a = ~m); the inner sum is
 *      accumulated from +0, corner b ascending, component j fastest; it is then multiplied by E_C; the cell terms are accumulated
 *      from +0.  A cell that does not exist counts as E = 0 with u = 0 on its missing nodes, which adds a zero.  No contraction.
 *      Diagonal D_{I,i} = sum_C E_C·K0[(a,i),(a,i)].  Right-hand side b_{I,i} = m_I·f_{I,i} with lsm_elliptic's node mass: a uniform
 *      traction t on a face normal to d is f = 2t/h_d on that face's nodes, the consistent load.
 *      Fixed components (fixed: one byte per node, bit i set = component i keeps u as passed; NULL: none, which is refused): clamped
 *      faces, rollers, symmetry planes.  Elimination as in lsm_elliptic: r0 = b − A u0 on the free components, search directions
 *      zero on the fixed ones.  A component without a fixed bit anywhere leaves its translation in the null space: refused.  A set
 *      that still leaves a rotation free (a single roller face, say) is the caller's to avoid: the solve then breaks down or does
 *      not converge, and says so.
 *      Hierarchy: lsm_elliptic's, per component (axis d coarsens while n_d > 5, to (n_d+1)/2 nodes; the same prolongation;
 *      restriction P^T/2^k; coarse cell moduli arithmetic means; the coarse operator the same discretisation with that level's K0;
 *      a coarse node's bits are fine node 2J's; residuals and corrections zero on fixed components on every level; the coarsest
 *      level, at most 125 nodes, runs 16 sweeps from zero).  Smoother: point Jacobi, 2 + 2 sweeps, the first from zero, with
 *      omega_l = min(0.6, 1.9/lambda_l) on level l — 0.6, not the scalar solve's 0.8, which is no convergent smoother for Q1
 *      elasticity in 3-D; lambda_l bounds lambda_max(D^−1 A) of the level on a uniform grid: the largest eigenvalue, over the 2^N
 *      corner frequencies theta in {0, pi}^N, of the N×N symbol D^−1/2·Ahat(theta)·D^−1/2 with Ahat_ij = sum_a sum_b s·K0[(a,i),(b,j)]
 *      (s = −1 where a and b differ on an odd number of the axes with theta_d = pi, else +1) and D_i = sum_a K0[(a,i),(a,i)]; it is
 *      2.86 on cubes and 2.22 on squares at nu = 0.3, where omega_l = 0.6.  Stretched cells — an axis that stopped coarsening while
 *      the others go on — push it past 2/0.6, where 0.6 would amplify and the V-cycle would be indefinite.  Point Jacobi still
 *      bounds the cell aspect ratio the V-cycle copes with: in 3-D its iteration count grows from max h/min h of about 1.5 on
 *      (DESIGN.md §7.18 has the counts), and from about 3 on the Jacobi preconditioner is the better choice.
 *      stats[4] (may be NULL) := {levels, free components, fixed components, 0}.  LSM_ERR_INVALID without running anything: a 1-D
 *      grid, a slab handle or one with a communicator, a periodic dimension, fewer than 3 nodes in a dimension, e_in / e_out not
 *      finite and positive, a bad nu, an unknown plane or precond.  LSM_ERR_INVALID after the setup kernel, with stats :=
 *      {−reason, offending entries, 0, 0}: a non-finite phi (1), a cell modulus not finite and positive (2), a component with no
 *      fixed bit (4; stats[1] := the component), everything fixed (5).
 *      lsm_elastic_apply: y = A x on all components, no elimination.  lsm_elastic_solve: f is N·nn fp64, component-major; u0, u1
 *      (, u2: NULL in 2-D) are N distinct dense fields of the handle: in, the guess and the prescribed values; out, the solution
 *      on the free components, rounded once to the storage type.  LSM_ERR_INVALID: a non-finite f or u.  LSM_ERR_NOT_CONVERGED:
 *      breakdown or max_iters.  In every failure u is untouched.
 *      lsm_elastic_energy: e_I = (sum over the existing cells C around I, ascending, of E_C·q_C)/(number of those cells),
 *      q_C = sum_r u_r·(sum_s K0[r,s]·u_s), both sums from +0 ascending over the cell's 2^N·N corner values: the cell mean of
 *      E·C0 ε:ε, the integrand of the compliance shape derivative; into a dense field of the handle, rounded once.
 *      lsm_elastic_compliance: *out := prod h · sum b·u, reduced on the device in workgroup order.
 *      lsm_elastic_cells copies the level-0 cell moduli into a device buffer.
 *      lsm_elastic_solve_many: K load cases of the one operator (1 <= K <= LSM_ELASTIC_MAXCOLS) solved in the same launches.
 *      Column k of the batch is lsm_elastic_solve of column k, bit for bit: the fields, the iteration count and the relative
 *      residual (every column has the single solve's launch shape, arithmetic and order, and its own device state).  f is
 *      K·N·nn fp64 on the device, column k at k·N·nn, component-major; u[k·N + i] is component i of column k, K·N distinct dense
 *      fields of the handle holding the guess and the prescribed values.  iters, relres and status are host arrays of K,
 *      filled for every column whatever the outcome; status: 1 converged, 2 out of iterations, −1 non-finite input, −2 breakdown
 *      (p·Ap not positive), −3 breakdown (r·Mr not positive, or a non-finite residual).  A column that has ended is skipped by
 *      its own workgroups while the others go on.  LSM_OK only when all columns converged, and only then are the free
 *      components of all columns stored; otherwise no field of any column changes, the converged ones included, and the error
 *      is LSM_ERR_INVALID if a column had non-finite input, else LSM_ERR_NOT_CONVERGED; the message names the lowest such column
 *      with its iterations and residual.  LSM_ERR_INVALID without running anything: K out of range, a null or repeated field,
 *      rtol not positive and finite, max_iters < 1.  The batch has a workspace of its own, allocated by the first call, kept on
 *      the object and grown when a later call asks for more columns; when it cannot be allocated the HIP error is returned and
 *      the object stays usable.  lsm_elastic_solve, the modes and the stress adjoint are unaffected by a batched call in
 *      between.  Not to be called concurrently with another call on the object.
 *      lsm_elastic_energy_many: e_I = sum_k w_k·e_{k,I}, k ascending from +0, e_{k,I} lsm_elastic_energy's value of column k in
 *      fp64 before its rounding; rounded once to the storage type, ghosts untouched; one pass over the grid.  LSM_ERR_INVALID:
 *      K out of range, a null or repeated field, an output that is an input, a weight that is not finite.
 *      lsm_elastic_energy_mutual: m_I = (sum over the existing cells C around I, ascending, of E_C·q_C)/(their number),
 *      q_C = sum_r u_r·(sum_s K0[r,s]·v_s), both sums from +0 in lsm_elastic_energy's order, rounded once: the integrand of the
 *      shape derivative of l·u for the state K u = f and the adjoint K v = l.  With v = u it is lsm_elastic_energy bit for bit.
 *      u and v may be the same fields; LSM_ERR_INVALID: a missing or repeated field within u or within v, an output that is an
 *      input. */
#define LSM_PLANE_STRESS 0
#define LSM_PLANE_STRAIN 1
typedef struct LsmElastic LsmElastic;
int lsm_elastic_create(LsmHandle* h, const void* phi, double level, double e_in, double e_out, const double* e_cells, double nu, int plane,
                       const void* fixed, int precond, LsmElastic** out, int64_t stats[4]);
int lsm_elastic_stiffness(LsmElastic* s, int level, double* k0_host);
int lsm_elastic_apply(LsmElastic* s, const double* x, double* y);
int lsm_elastic_solve(LsmElastic* s, const double* f, void* u0, void* u1, void* u2, double rtol, int max_iters, int* iters, double* relres,
                      void* stream);
int lsm_elastic_energy(LsmElastic* s, const void* u0, const void* u1, const void* u2, void* e_out);
int lsm_elastic_compliance(LsmElastic* s, const double* f, const void* u0, const void* u1, const void* u2, double* out);
int lsm_elastic_cells(LsmElastic* s, double* e_out_cells);
#define LSM_ELASTIC_MAXCOLS 8
int lsm_elastic_solve_many(LsmElastic* s, int K, const double* f, void* const* u, double rtol, int max_iters, int* iters, double* relres,
                           int* status, void* stream);
int lsm_elastic_energy_many(LsmElastic* s, int K, void* const* u, const double* w, void* e_out);
int lsm_elastic_energy_mutual(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* v0, const void* v1, const void* v2,
                              void* e_out);
void lsm_elastic_destroy(LsmElastic* s);

/* ---- homogenize: the effective elasticity tensor C^H of the periodic material whose cell is the box of a dense 2-D or 3-D grid,
 *      and its sensitivity (csrc/lsm_homog.hip; tests/_homog_ref.py restates every operation).  Shapes, ownership,
 *      streams and failures are lsm_elastic_*'s unless stated.
 *      The torus.  m_d = n_d − 1 cells per axis; the period is m_d cells, node n_d − 1 is node 0 (the reference's periodic
 *      convention, src/boundaryconditions.jl:107-119).  The unknowns live on the nn = m_0·m_1(·m_2) nodes of the torus, id = I0 +
 *      m0·(I1 + m1·I2); cell C (lowest corner C) has the same linear index.  Every node has all 2^N cells around it: cell index
 *      I_d − 1 wraps to m_d − 1, corner C_d + 1 wraps to 0.  The handle's boundary conditions are not read: only phi's cells are.
 *      Cell moduli, the material, plane and K0: lsm_elastic's, the same code and the same bits; the cell array is n − 1-shaped.
 *      Operator: lsm_elastic's sums in lsm_elastic's order over the wrapped cells and nodes; no cell is missing.  Diagonal likewise.
 *      Unit strains, M = N(N+1)/2, in Voigt order: 2-D (00, 11, 01); 3-D (00, 11, 22, 12, 02, 01); shears are engineering shears
 *      gamma = 1.  The cell-local affine field chi0^k at a cell's corners (corner a at x_d = bit_d(a)·h_d): normal strain ii:
 *      component i = x_i; shear ij: component i = x_j/2, component j = x_i/2; all else zero.  g^k = K0·chi0^k, each row summed from
 *      +0 ascending, on the host.  Load: f^k_{I,i} = −(sum over the cells C around I, ascending as in the operator, from +0, of
 *      E_C·g^k[(a, i)]), a = I's corner in C.  lsm_homog_load writes all N·nn entries, node 0's included.
 *      Correctors: chi^k is periodic with its N components zero at node 0 (the pin) and solves A chi^k = f^k on the others, by
 *      lsm_elastic's PCG (b = f^k: no node mass on a torus).  w^k_C = chi0^k + chi^k at the corners of C;
 *      t^{pq}_C = E_C·(sum_r w^p_r·(sum_s K0[r,s]·w^q_s)), both sums from +0 ascending; C^H_pq = (sum_C t^{pq}_C)/ncells (K0 carries
 *      1/prod h: the mean energy density).  lsm_homog_tensor forms K0·w^q once per q and the sums for p ≤ q in one pass, reduced in
 *      workgroup order, and mirrors them: C is M·M doubles on the host, exactly symmetric, and two calls give the same bits.
 *      Hierarchy: axis d coarsens while m_d is even and m_d > 4, to m_d/2 with 2h; it ends when no axis coarsens.  A coarse cell is
 *      the mean of cells 2J and 2J+1 per coarsened axis (lsm_elastic's average).  Restriction r_c[J] = 2^−k·sum_o w_o·res[(2J + o)
 *      mod m], w = 1 at o = 0 and 1/2 at o = ±1 per coarsened axis; prolongation its transpose without the 2^−k.  Node 0 is pinned
 *      on every level.  omega_l = min(0.6, 1.9/lambda_l) as in lsm_elastic.  Smoother 2 + 2 sweeps; the coarsest level runs 16
 *      sweeps from zero: in one workgroup with at most 128 nodes, else (an odd m_d on a large axis) as 16 launches of the smoother,
 *      the same arithmetic.  No shape is refused but an axis with m_d < 2.
 *      stats[4] (may be NULL) := {levels, free components, nodes of the torus, 0}; after the setup kernel refused the data
 *      {−reason, offending entries, 0, 0}: a non-finite phi (1, counted over all n nodes), a cell modulus not finite and
 *      positive (2).  LSM_ERR_INVALID without running anything: a 1-D grid, a slab handle or one with a communicator, fewer than 3
 *      nodes in a dimension, bad e_in / e_out / level / nu / plane / precond.
 *      lsm_homog_apply: y = A x over N·nn device doubles, component-major, no pin.  lsm_homog_cells: the cell moduli, device.
 *      lsm_homog_solve: all M correctors from chi_guess (M·N·nn fp64, host or device; node 0's entries are taken as zero; NULL:
 *      from zero); iters[M] and relres[M] (may be NULL) per corrector.  The stored correctors change only when all M solves have
 *      converged: LSM_ERR_NOT_CONVERGED or a non-finite guess (LSM_ERR_INVALID) leaves them untouched, with iters and relres set up
 *      to the solve that failed.  A new object holds zero correctors.  lsm_homog_set_correctors / lsm_homog_correctors copy all of
 *      them from / to fp64 memory of the caller (host or device), shape (M, N) + m.
 *      lsm_homog_solve_rhs: the same PCG for a caller's right-hand side, A x = f away from the pin (f, x: N·nn device doubles; x in:
 *      the guess, node 0's entries taken as zero; out: the solution); the stored correctors are not touched, and a failure leaves x
 *      untouched.  For diagnostics and tests of the V-cycle.
 *      lsm_homog_energy_cells: t^{pq}_C of every cell into ncells device doubles, from the stored correctors.
 *      lsm_homog_corrector: chi^k into N distinct dense fields of the handle, image nodes n − 1 from node 0, rounded once.
 *      lsm_homog_sensitivity: W is M·M host doubles, finite and symmetric.  cell_C = sum_q sum_{p ≤ q} c·W[p·M + q]·t^{pq}_C, c = 2
 *      for p < q and 1 for p = q (the tensor's own pairs: t^{qp} is t^{pq}), q ascending and within it p ascending, from +0, the
 *      product as (c·W)·t (K0·w^q once per q); g_I = (sum over the cells C around I, ascending,
 *      from +0, of cell_C)·2^−N at every node of the handle's grid (node n − 1 is node 0), rounded once into a dense field: the
 *      integrand of d(W:C^H)/dOmega in lsm_elastic_energy's node-mean convention. */
typedef struct LsmHomog LsmHomog;
int lsm_homog_create(LsmHandle* h, const void* phi, double level, double e_in, double e_out, const double* e_cells, double nu, int plane,
                     int precond, LsmHomog** out, int64_t stats[4]);
int lsm_homog_stiffness(LsmHomog* s, int level, double* k0_host);
int lsm_homog_cells(LsmHomog* s, double* e_out_cells);
int lsm_homog_apply(LsmHomog* s, const double* x, double* y);
int lsm_homog_load(LsmHomog* s, int k, double* f_out);
int lsm_homog_solve(LsmHomog* s, const double* chi_guess, double rtol, int max_iters, int* iters, double* relres);
int lsm_homog_solve_rhs(LsmHomog* s, const double* f, double* x, double rtol, int max_iters, int* iters, double* relres);
int lsm_homog_set_correctors(LsmHomog* s, const double* chi);
int lsm_homog_correctors(LsmHomog* s, double* chi_out);
int lsm_homog_energy_cells(LsmHomog* s, int p, int q, double* out);
int lsm_homog_tensor(LsmHomog* s, double* C);
int lsm_homog_corrector(LsmHomog* s, int k, void* u0, void* u1, void* u2);
int lsm_homog_sensitivity(LsmHomog* s, const double* W, void* g_out);
void lsm_homog_destroy(LsmHomog* s);

/* ---- homogenize_conductivity: the effective conductivity tensor K^H of −div(a grad u) for the periodic material whose cell is the
 *      box of a dense 2-D or 3-D grid, and its sensitivity (csrc/lsm_hcond.hip; tests/_hcond_ref.py restates every
 *      operation).  Shapes, ownership, streams and failures are lsm_homog_*'s unless stated; every sum below starts from +0.
 *      The torus: lsm_homog's.  m_d = n_d − 1 nodes and cells per axis, node n_d − 1 is node 0, id = I0 + m0·(I1 + m1·I2) for node I
 *      and for cell I (lowest corner I); cell index I_d − 1 wraps to m_d − 1, node I_d + 1 wraps to 0.  The handle's boundary
 *      conditions are not read: only phi's cells are.  Cell coefficients: lsm_elliptic's formula, code and bits (a_cells != NULL:
 *      the caller's n − 1-shaped device array, phi may be NULL).
 *      Operator: lsm_elliptic's edge form with wrapping neighbours and c = 0.  The 2^N cells around node I are numbered m = 0 …
 *      2^N − 1, bit d of m set: cell I_d along d, clear: cell I_d − 1.  The edge from I towards I ± e_d has kbar = (sum of the
 *      2^(N−1) cells whose bit d is 1 (plus) or 0 (minus), m ascending)·(1/2 in 2-D, 1/4 in 3-D), and w = kbar·ih2_d, ih2_d =
 *      1/(h_d·h_d).  (A x)_I = sum over d ascending, the minus side before the plus side, of w·(x_I − x_J).  There is no node mass,
 *      no missing cell and no face.  The diagonal D_I: the sum of the w in the same order.
 *      Cell problems, p = 0 … N−1 (the unit gradient e_p): the load f^p_I = kbar(I → I + e_p)/h_p − kbar(I − e_p → I)/h_p;
 *      chi^p is periodic, zero at node 0 (the pin), and solves A chi^p = f^p on the other nodes by lsm_elliptic's PCG (b = f^p).
 *      lsm_hcond_load writes all nn entries, node 0's included.
 *      Cell integrand, for cell C with corners a = 0 … 2^N − 1 (corner a at C + bits(a), wrapped): on the edge along d that starts
 *      at a corner a whose bit d is clear, g^p_{d,a} = delta_dp + (chi^p[a + e_d] − chi^p[a])/h_d (delta is 1.0 or 0.0, added
 *      first).  t^{pq}_C = (a_C·2^−(N−1))·(sum over d ascending, within it a ascending, of g^p_{d,a}·g^q_{d,a}).
 *      K^H_pq = (sum_C t^{pq}_C)/ncells.  lsm_hcond_tensor forms the N(N+1)/2 sums for p ≤ q in one pass over the cells, reduced in
 *      workgroup order, and mirrors them: K is N·N doubles on the host, exactly symmetric, and two calls give the same bits.
 *      Hierarchy and transfers: lsm_homog's (axis d coarsens while m_d is even and m_d > 4; a coarse cell is the mean of cells 2J
 *      and 2J+1 per coarsened axis; the wrapping restriction and prolongation; node 0 pinned on every level), with ih2 from the
 *      level's own h.  omega = 0.8, lsm_elliptic's.  Smoother 2 + 2 sweeps; the coarsest level runs 16 sweeps from zero: in one
 *      workgroup with at most 128 nodes, else as 16 launches of the smoother, the same arithmetic.  No shape is refused but an axis
 *      with m_d < 2.
 *      stats[4] (may be NULL) := {levels, free nodes (nn − 1), nodes of the torus, 0}; after the setup kernel refused the data
 *      {−reason, offending entries, 0, 0}: a non-finite phi (1, counted over all n nodes), a cell coefficient not finite and
 *      positive (2).  LSM_ERR_INVALID without running anything: a 1-D grid, a slab handle or one with a communicator, fewer than 3
 *      nodes in a dimension, bad a_in / a_out / level / precond.
 *      lsm_hcond_apply: y = A x over nn device doubles, no pin.  lsm_hcond_cells: the cell coefficients, device.
 *      lsm_hcond_solve: all N correctors from chi_guess (N·nn fp64, host or device; node 0's entries are taken as zero; NULL: from
 *      zero); iters[N] and relres[N] (may be NULL) per corrector.  The correctors are fp64 on the device on a float32 handle too,
 *      and change only when all N solves have converged: LSM_ERR_NOT_CONVERGED or a non-finite guess (LSM_ERR_INVALID) leaves them
 *      untouched, with iters and relres set up to the solve that failed.  A new object holds zero correctors.
 *      lsm_hcond_set_correctors / lsm_hcond_correctors copy all of them from / to fp64 memory of the caller (host or device),
 *      shape (N,) + m.
 *      lsm_hcond_solve_rhs: the same PCG for a caller's right-hand side, A x = f away from the pin (f, x: nn device doubles; x in:
 *      the guess, node 0's entry taken as zero; out: the solution); the stored correctors are not touched, and a failure leaves x
 *      untouched.  For diagnostics and tests of the V-cycle.
 *      lsm_hcond_energy_cells: t^{pq}_C of every cell into ncells device doubles, from the stored correctors.
 *      lsm_hcond_corrector: chi^k into a dense field of the handle, image nodes n − 1 from node 0, rounded once.
 *      lsm_hcond_sensitivity: W is N·N host doubles, finite and symmetric.  cell_C = sum_q sum_{p ≤ q} (c·W[p·N + q])·t^{pq}_C,
 *      c = 2 for p < q and 1 for p = q, q ascending and within it p ascending; g_I = (sum over the 2^N cells around I, m
 *      ascending, of cell_C)·2^−N at every node of the handle's grid (node n − 1 is node 0), rounded once into a dense field: the
 *      integrand of d(W:K^H)/dOmega in lsm_homog_sensitivity's node-mean convention. */
typedef struct LsmHcond LsmHcond;
int lsm_hcond_create(LsmHandle* h, const void* phi, double level, double a_in, double a_out, const double* a_cells, int precond, LsmHcond** out,
                     int64_t stats[4]);
int lsm_hcond_cells(LsmHcond* s, double* a_out_cells);
int lsm_hcond_apply(LsmHcond* s, const double* x, double* y);
int lsm_hcond_load(LsmHcond* s, int k, double* f_out);
int lsm_hcond_solve(LsmHcond* s, const double* chi_guess, double rtol, int max_iters, int* iters, double* relres);
int lsm_hcond_solve_rhs(LsmHcond* s, const double* f, double* x, double rtol, int max_iters, int* iters, double* relres);
int lsm_hcond_set_correctors(LsmHcond* s, const double* chi);
int lsm_hcond_correctors(LsmHcond* s, double* chi_out);
int lsm_hcond_energy_cells(LsmHcond* s, int p, int q, double* out);
int lsm_hcond_tensor(LsmHcond* s, double* K);
int lsm_hcond_corrector(LsmHcond* s, int k, void* u);
int lsm_hcond_sensitivity(LsmHcond* s, const double* W, void* g_out);
void lsm_hcond_destroy(LsmHcond* s);

/* ---- elasticity_modes: the m smallest eigenpairs of A x = lambda·M x for the ersatz-material structure of an LsmElastic — its
 *      vibration modes, lambda = omega² — by a locally optimal block preconditioned CG (LOBPCG) whose preconditioner T is the
 *      object's V-cycle, or 1/D for LSM_PRECOND_JACOBI (csrc/lsm_elastic.hip; tests/_modes_ref.py restates it).
 *      A is lsm_elastic_apply's operator, scaled by 1/prod h as it is, with the fixed components eliminated: they are zero in
 *      every mode, whatever values a solve prescribes there.  The fixed set must hold every rigid-body motion.
 *      Mass: lumped, the same for every component of a node.  Cell density rho_C = lsm_elliptic's cell formula with (rho_in,
 *      rho_out) for (a_in, a_out) — the code and the fill fraction of the modulus — or rho_cells != NULL: the caller's cell array,
 *      n−1 per axis, on the device (phi may be NULL then).  M_I = (sum of rho_C over the existing cells around I, ascending
 *      m = 0 … 2^N−1, from +0)·2^−N: M is scaled by 1/prod h like A, so lambda needs no factor.  rho_out/rho_in must stay far below
 *      e_out/e_in, or the lowest modes are spurious ones living in the ersatz material.
 *      Vectors: a block has m columns of N·nn fp64, column-major, a column component-major as lsm_elastic_apply's x.  The object
 *      holds X, W, P and A·X, A·W, A·P: 6·m·N·nn doubles, plus the node mass and the cell densities.
 *      Start: x0 (device, m·N·nn doubles), or NULL: entry t = k·N·nn + i·nn + id takes z = t + 0x9E3779B97F4A7C15 (mod 2^64),
 *      z = (z ^ z>>30)·0xBF58476D1CE4E5B9, z = (z ^ z>>27)·0x94D049BB133111EB, z = z ^ z>>31 (splitmix64), d = (z>>11)·2^−53, the
 *      value 2d − 1.  Either way the fixed components are set to zero.  A·X = A X once; then one Rayleigh–Ritz step on span X.
 *      Iteration, with lambda_k the Ritz values:
 *        1. R_k = A·X_k − lambda_k·(M·X_k) for every k, and ‖R_k‖₂, ‖M·X_k‖₂.  Column k has converged when ‖R_k‖₂ <=
 *           rtol·lambda_k·‖M·X_k‖₂; relres[k] = ‖R_k‖₂/(lambda_k·‖M·X_k‖₂).  All converged: done.  iters == max_iters: not converged.
 *        2. W_j = T(R_k), A·W_j = A W_j for the na columns k that have not converged, ascending (soft locking: a converged column
 *           stays in X and is rotated with it, but gives no W or P column).
 *        3. Gram matrices G_A = S^T (A·S), G_M = S^T (M·S) over S = [X, W, P], q = m + na + np <= 24 columns (np = the previous
 *           iteration's na; 0 at first).  Only entries i <= j are formed and mirrored.  Entry (i, j) is a sum over the N·nn rows of
 *           S_i·(A·S)_j, or of S_i·(M·S_j), multiply then add: each thread over its rows ascending (row = thread + k·threads), then the
 *           wave butterfly, the workgroup's waves as (0+1)+(2+3), and the workgroups in order; the launch is a function of the grid
 *           alone, so two solves from the same start return the same bits.
 *        4. Rayleigh–Ritz on the host, fp64, cyclic Jacobi: s_i = G_M[i,i]^−1/2; G'_M = s G_M s, G'_A = s G_A s; (mu, V) the
 *           eigen-decomposition of G'_M; directions with mu <= 1e-12·max mu are dropped; B = V·mu^−1/2; (theta, Z) the
 *           eigen-decomposition of B^T G'_A B, ascending; C = s·B·Z[:, 0…m−1], lambda = theta[0…m−1].
 *        5. X <- S·C and A·X <- (A·S)·C; P <- [W, P]·C' and A·P <- [A·W, A·P]·C', C' = the W and P rows of C and the columns of the
 *           na unconverged k.  Row by row, each sum from +0 over the columns of S ascending, multiply then add.  A·X and A·P are
 *           never recomputed.  X leaves every iteration M-orthonormal.
 *      lsm_elastic_modes_solve: lambda, relres (host, m doubles each), iters (block iterations) and stats (may be NULL) :=
 *      {iterations, preconditioner applications, directions dropped, unconverged columns} are written in every return that ran.
 *      LSM_ERR_INVALID without running anything: m outside 1 … 8, 3·m above the free components, rho_in / rho_out not finite and
 *      positive, a non-finite level (create); rtol not positive and finite, max_iters < 1 (solve).  LSM_ERR_INVALID after a
 *      kernel: a non-finite phi or a cell density not finite and positive (create), a non-finite x0 (solve).
 *      LSM_ERR_NOT_CONVERGED: max_iters did not suffice, or a Gram matrix (or the preconditioner) is not positive; X is the last
 *      iterate then, and vectors, store and sensitivity work on it.  The second happens where 3·m comes close to the number of free
 *      components (5 modes of 16 unknowns, say): S then nearly spans the whole space, its Gram matrix loses rank as columns
 *      converge, and the reduced problem is no longer positive to rounding.  Such problems are a dense solver's.
 *      lsm_elastic_modes_mass copies the node mass (nn doubles), lsm_elastic_modes_vectors X (m·N·nn doubles) into device buffers.
 *      lsm_elastic_modes_store: mode k into N distinct dense fields of the handle: X_k·(prod h)^−1/2 rounded once to the storage
 *      type, so that prod h·sum M·|u|² = 1, the discrete ∫rho·|u|² = 1; exact zeros on the fixed components; ghosts untouched.  The
 *      sign of a mode is not specified.
 *      lsm_elastic_modes_sensitivity: g_I = e_I − (lambda_k·rhobar_I)·(sum_i u_{I,i}², from +0, i ascending) into a dense field,
 *      rounded once: u the stored mode (rounded to the storage type), e_I lsm_elastic_energy's value of u in fp64 before its
 *      rounding, rhobar_I = (sum of rho_C over the existing cells around I, ascending from +0)/(their number).  It is the integrand
 *      of the shape derivative of lambda_k, a normal speed.
 *      The modes object borrows the LsmElastic, which must outlive it, and uses its scratch vectors: a solve of either must not run
 *      concurrently with the other, and lsm_elastic_solve's results are unaffected by a modes solve in between. */
typedef struct LsmModes LsmModes;
int lsm_elastic_modes_create(LsmElastic* s, const void* phi, double level, double rho_in, double rho_out, const double* rho_cells, int m,
                             LsmModes** out);
int lsm_elastic_modes_mass(LsmModes* md, double* node_mass);
int lsm_elastic_modes_solve(LsmModes* md, const double* x0, double rtol, int max_iters, double* lambda, double* relres, int* iters,
                            int64_t stats[4]);
int lsm_elastic_modes_vectors(LsmModes* md, double* x_out);
int lsm_elastic_modes_store(LsmModes* md, int k, void* u0, void* u1, void* u2);
int lsm_elastic_modes_sensitivity(LsmModes* md, int k, void* g_out);
void lsm_elastic_modes_destroy(LsmModes* md);

/* ---- elliptic_modes: the m smallest eigenpairs of A x = lambda·M x for the scalar operator of an LsmElliptic — the resonances of a
 *      cavity, the tones of a membrane, the principal eigenvalue of a diffusion problem — by the LOBPCG of "elasticity_modes" above
 *      with one component per node: the same core (csrc/lobpcg.h), the same iteration, steps 1 … 5, the same Rayleigh–Ritz, stop test,
 *      returns and stats (csrc/lsm_elliptic.hip; tests/_emodes_ref.py restates it).  What differs:
 *      A is lsm_elliptic_apply's operator, its c term included, scaled by 1/prod h as it is, with the fixed nodes eliminated: they are
 *      zero in every mode.  A must be positive definite; lsm_elliptic_create refuses "no fixed node and c = 0", so a cavity with natural
 *      walls only needs c > 0.  With a constant c and rho == 1 the spectrum is that of c = 0 shifted by exactly c (M_I is then
 *      the node mass m_I of "elliptic_solve", bit for bit); in general the pencil is (K + c·m, M).  An exact spectral shift is not
 *      offered.
 *      Mass: M_I = (sum of rho_C over the existing cells around I, ascending, from +0)·2^−N, rho_C as for elasticity_modes (the cell
 *      formula with (rho_in, rho_out), or rho_cells).  rho_out/rho_in must stay far below a_out/a_in.
 *      Vectors: a block has m columns of nn fp64, column-major; the object holds 6·m·nn doubles plus the node mass and the cell
 *      densities.  Start: x0 (device, m·nn doubles), or NULL: entry t = k·nn + id takes the splitmix64 value of elasticity_modes.
 *      The fixed nodes are set to zero either way.
 *      The preconditioner is one V-cycle of the LsmElliptic per unconverged column, or 1/D for LSM_PRECOND_JACOBI.
 *      lsm_elliptic_modes_apply: y_k = A x_k for ncols (1 … 8, else LSM_ERR_INVALID) columns of nn doubles on the device, x zero on
 *      the fixed nodes: the rows of fixed nodes are zero, fixed neighbours count as zero, and every column has the bits of
 *      lsm_elliptic_apply's arithmetic in its order.  It is the solve's block apply, exported so that tests can see it.
 *      LSM_ERR_INVALID as for elasticity_modes with "free nodes" for "free components" (3·m above the free nodes).
 *      lsm_elliptic_modes_store: mode k into one dense field: X_k·(prod h)^−1/2 rounded once to the storage type, so that
 *      prod h·sum M·u² = 1; exact zeros on the fixed nodes; ghosts untouched.  The sign of a mode is not specified.
 *      lsm_elliptic_modes_sensitivity: g_I = e_I − (lambda_k·rhobar_I)·(u_I·u_I) into a dense field, rounded once: u the stored mode
 *      (rounded to the storage type), e_I lsm_elliptic_energy's value of u in fp64 before its rounding, rhobar_I = (sum of rho_C over
 *      the existing cells around I, ascending from +0)/(their number).  c does not move with the shape and gives no term.  For a
 *      membrane whose outside nodes are fixed the shape derivative is a boundary flux, not this integrand.
 *      The modes object borrows the LsmElliptic, which must outlive it, and uses its scratch vectors and its state: a solve of either
 *      must not run concurrently with the other, and lsm_elliptic_solve's results are bit-identical with or without a modes solve in
 *      between. */
typedef struct LsmEllipticModes LsmEllipticModes;
int lsm_elliptic_modes_create(LsmElliptic* s, const void* phi, double level, double rho_in, double rho_out, const double* rho_cells, int m,
                              LsmEllipticModes** out);
int lsm_elliptic_modes_mass(LsmEllipticModes* md, double* node_mass);
int lsm_elliptic_modes_apply(LsmEllipticModes* md, int ncols, const double* x, double* y);
int lsm_elliptic_modes_solve(LsmEllipticModes* md, const double* x0, double rtol, int max_iters, double* lambda, double* relres, int* iters,
                             int64_t stats[4]);
int lsm_elliptic_modes_vectors(LsmEllipticModes* md, double* x_out);
int lsm_elliptic_modes_store(LsmEllipticModes* md, int k, void* u);
int lsm_elliptic_modes_sensitivity(LsmEllipticModes* md, int k, void* g_out);
void lsm_elliptic_modes_destroy(LsmEllipticModes* md);

/* ---- stress recovery: the cell-mean strain and stress of a displacement u on an LsmElastic, the von Mises field, the p-norm
 *      aggregate of the von Mises stress with its adjoint load and its sensitivity to the cell moduli — the stress objective of a
 *      structural shape optimisation (csrc/lsm_elastic.hip; tests/_stress_ref.py restates every operation).  u0,
 *      u1 (, u2: NULL in 2-D) are N distinct dense fields of the handle; any displacement, not only a solution.  No contraction;
 *      every sum below starts from +0 and runs in the stated order.
 *      Setting: a cell C has the corners b = 0 … 2^N−1, bit d of b set on the upper side along d; u_{b,i} the corner values, converted
 *      to fp64 first on a float32 handle; c_j = (1/h_j)·2^−(N−1), computed on the host in fp64; lambda, mu the object's material at
 *      E = 1 (plane-dependent); E_C the cell modulus.
 *      Cell-mean gradient: d_ij = sum_b (bit j of b set ? u_{b,i} : −u_{b,i}), b ascending; G_ij = d_ij·c_j — the gradient at the
 *      centroid, the superconvergent point of Q1.
 *      Voigt order: 2-D (00, 11, 01); 3-D (00, 11, 22, 12, 02, 01); M = N(N+1)/2 components.
 *      Strain: e_ii = G_ii; e_ij = G_ij + G_ji for i < j (engineering shear).  tr = G_00 + G_11 (+ G_22), left to right.
 *      Unit stress: shat_ii = lambda·tr + (2·mu)·G_ii; tauhat_ij = mu·e_ij; in 2-D the out-of-plane normal stress shat_zz = lambda·tr
 *      for LSM_PLANE_STRAIN and 0 for LSM_PLANE_STRESS.  The stress is E_C·shat, E_C·tauhat: the ersatz modulus relaxes it in the void.
 *      Von Mises: with (a, b, c) = (shat_00, shat_11, shat_22 or shat_zz), v2 = 0.5·(((a−b)² + (b−c)²) + (c−a)²) + 3·(sum of tauhat²,
 *      Voigt order); t_C = sqrt(v2); s_C = E_C·t_C.
 *      Node fields: the value at node I is (sum of the cell values over the existing cells around I, ascending m as in
 *      lsm_elastic_energy)/(their number), rounded once to the storage type; ghosts untouched.
 *      Aggregate, for 2 <= p <= 64 and sref > 0: r_C = s_C/sref, J' = sum_C pow(r_C, p), each thread over its cells ascending (cell =
 *      thread + k·threads), then the ordered workgroup reduction of the solver; smax = max_C s_C in the same pass.  The p-norm is
 *      G_p = sref·(prod h·J')^(1/p), left to the caller.
 *      Adjoint load g = dJ'/du, gathered without atomics: g_{I,i} = sum over the existing cells C around I, ascending, of
 *      w_C·(sum_j ±(c_j·Z_ij(C)), j ascending), + where I is on C's upper side along j.  w_C = (p·((E_C/sref)·(E_C/sref)))·pow(r_C, p−2),
 *      which has no singularity where the strain vanishes (hence p >= 2).  m_k = shat_k − 0.5·(shat_l + shat_n) over the three normal
 *      stresses (l < n the other two; the third is shat_zz in 2-D); Z_ii = lambda·(sum of m_k over the normal stresses that depend on
 *      the strain: (m_0 + m_1) + m_2 in 3-D and for plane strain, m_0 + m_1 for plane stress) + (2·mu)·m_i; Z_ij = Z_ji = (3·mu)·tauhat_ij.
 *      What is written is f = g/m_I with lsm_elliptic's node mass, a power of two: lsm_elastic_solve takes it unchanged, b = m·f = g.
 *      Sensitivity: with the solution a of A a = g on the free components, zero on the fixed ones, given as N fields l0, l1 (, l2),
 *      d_I = (scale·(sum over the existing cells around I, ascending, of p·pow(r_C, p) − E_C·(sum_r a_r·(sum_s K0[r,s]·u_s))))/(their
 *      number), the bilinear form in lsm_elastic_energy's order, rounded once.  Cell by cell the summand is E_C·dJ'/dE_C, exact for
 *      the discrete problem, prescribed non-zero displacements included; with scale = G_p/(p·J') it is E_C·dG_p/dE_C, the convention
 *      of lsm_elastic_energy: positive where more material raises G_p.  With zero prescribed values sum_I count_I·d_I = 0.
 *      lsm_elastic_stress_cells: component-major fp64 cell arrays on the device (n−1 per axis, axis 0 fastest): the M components for
 *      LSM_STRESS_STRAIN and LSM_STRESS_STRESS, s_C for LSM_STRESS_VON_MISES.  lsm_elastic_stress: the node fields into distinct
 *      dense fields of the handle, o0 … o(M−1) (NULL past the last; LSM_STRESS_VON_MISES writes o0 only).  lsm_elastic_stress_norm:
 *      out := {J', smax}, synchronous; a NaN stress makes both NaN.  lsm_elastic_stress_load: f, N·nn fp64 on the device,
 *      component-major.  lsm_elastic_stress_sensitivity: d into the dense field g_out.
 *      LSM_ERR_INVALID without running anything: an unknown `what`, p outside [2, 64], sref not positive and finite, scale not finite,
 *      a missing or repeated field, an output that is one of the inputs.  A non-finite u propagates, as in lsm_elastic_energy.
 *      The calls use the object's scratch vectors (but lsm_elastic_stress_cells, which writes the caller's array only): none must run
 *      concurrently with a solve of the object or of its modes, and the results of a later lsm_elastic_solve or
 *      lsm_elastic_modes_solve are unaffected by them. */
#define LSM_STRESS_STRAIN 0
#define LSM_STRESS_STRESS 1
#define LSM_STRESS_VON_MISES 2
int lsm_elastic_stress_cells(LsmElastic* s, const void* u0, const void* u1, const void* u2, int what, double* out);
int lsm_elastic_stress(LsmElastic* s, const void* u0, const void* u1, const void* u2, int what, void* o0, void* o1, void* o2, void* o3, void* o4,
                       void* o5);
int lsm_elastic_stress_norm(LsmElastic* s, const void* u0, const void* u1, const void* u2, double p, double sref, double out[2]);
int lsm_elastic_stress_load(LsmElastic* s, const void* u0, const void* u1, const void* u2, double p, double sref, double* f_out);
int lsm_elastic_stress_sensitivity(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* l0, const void* l1, const void* l2,
                                   double p, double sref, double scale, void* g_out);

/* ---- topological derivative of the compliance (Garreau, Guillaume & Masmoudi 2001; Allaire, de Gournay, Jouve & Toader 2005): T is
 *      the cost per unit volume removed — a small traction-free hole of volume v around x raises lsm_elastic_compliance by about
 *      T(x)·v — computed from the cell strain and unit stress of the stress recovery above, whose setting, notation and Voigt order
 *      it shares (csrc/lsm_elastic.hip; tests/_topo_ref.py restates every operation).  No contraction; every sum
 *      starts from +0 and runs in the stated order.
 *      w = shat : e = sum_i shat_ii·G_ii (i ascending), continued by sum over the shears of tauhat_ij·e_ij in Voigt order, one
 *      accumulator.  tr = G_00 + G_11 (+ G_22); trs = shat_00 + shat_11 (+ shat_22), left to right: in 2-D the in-plane traces, also for
 *      LSM_PLANE_STRAIN (shat_zz stays out).  T_C = E_C·(a·w + b·(trs·tr)).
 *      a and b come from lambda, mu (the object's material at E = 1, plane-dependent) once, on the host, in fp64:
 *      N = 2: g = (lambda + 2·mu)/((2·mu)·(lambda + mu)), a = g·(4·mu), b = g·(lambda − mu);
 *      N = 3: g = (3·(lambda + 2·mu))/((4·mu)·(9·lambda + 14·mu)), a = g·(20·mu), b = g·(3·lambda − 2·mu)
 *      — the polarisation of a circular / spherical void divided by the volume of the unit ball (pi, 4·pi/3).  In plane stress
 *      T = ((s1 + s2)² + 2·(s1 − s2)²)/E in the principal stresses; in plane strain (1 − nu²) times that; in 3-D
 *      3(1 − nu)/(2(7 − 5nu))·(10·s:e − (1 − 5nu)/(1 − 2nu)·tr(s)·tr(e)).  The formula is the void's: the ersatz modulus of the
 *      outside is taken for void, and T_C there is small like E_C.  T_C >= 0 and T_C >= E_C·w.
 *      lsm_elastic_topo_cells: one fp64 cell array on the device (n−1 per axis, axis 0 fastest).  lsm_elastic_topo: the node field
 *      into the dense field o0 by the stress recovery's rule — (sum of T_C over the existing cells around I, ascending m, from
 *      +0)/(their number), rounded once to the storage type; ghosts untouched.
 *      LSM_ERR_INVALID without running anything: a missing or repeated field of u, an output that is missing or one of the inputs.
 *      A non-finite u propagates.  lsm_elastic_topo uses the object's scratch vectors as lsm_elastic_stress does: it must not run
 *      concurrently with a solve of the object or of its modes, and the results of a later solve are unaffected. */
int lsm_elastic_topo_cells(LsmElastic* s, const void* u0, const void* u1, const void* u2, double* out);
int lsm_elastic_topo(LsmElastic* s, const void* u0, const void* u1, const void* u2, void* o0);

/* ---- thermoelastic coupling: a temperature field T as a load on the structure of an LsmElastic, the stress with the thermal strain
 *      taken off, the elastic adjoint carried back into the heat problem, and the sensitivity of l·u to the cell moduli with the
 *      thermal load in it (csrc/lsm_elastic.hip; tests/_thermo_ref.py restates every operation).  The setting is the
 *      stress recovery's: the corners b of a cell C, c_j, lambda, mu, E_C, and tr_C(v) = G_00 + G_11 (+ G_22), the cell-mean divergence
 *      of a displacement v, formed exactly as there.  Everything is fp64 without contraction; every sum starts from +0 and runs in the
 *      stated order; a float32 handle converts its fields to fp64 first and rounds an output field once.  T, u, v and minus are dense
 *      fields of the handle.
 *      beta = 3·lambda + 2·mu in 3-D and for LSM_PLANE_STRAIN, 2·lambda + 2·mu for LSM_PLANE_STRESS — 1/(1−2nu) and 1/(1−nu) —
 *      computed once on the host.  ab_C = alpha_C·beta, alpha_C = alpha_cells[C] (n−1 per axis, axis 0 fastest, fp64 on the device)
 *      or, with alpha_cells == NULL, the scalar alpha (which is not read otherwise).  theta_C = (sum_b T_b, b ascending)·2^−N − t_ref.
 *      t_C = ab_C·theta_C, the unit thermal stress; g_C = E_C·t_C.
 *      lsm_elastic_thermal_load: b_{I,i} = sum over the existing cells C around I, ascending m, of ±(c_i·g_C), + where I is on C's
 *      upper side along i (bit i of m clear); f = b/m_I is written, N·nn fp64 on the device, component-major: the form
 *      lsm_elastic_solve takes, as lsm_elastic_stress_load writes it.  It is the consistent Q1 load of the eigenstress
 *      E·C0:(alpha·theta·I) with theta taken at the centroid, so that A u = b_m + b_th is the thermally loaded state; with uniform E,
 *      alpha and theta the free expansion u_i = eps·x_i, eps = alpha·theta (3-D, plane stress) or (1+nu)·alpha·theta (plane strain),
 *      satisfies A u = b_th on every node to rounding.
 *      lsm_elastic_thermal_stress_cells, lsm_elastic_thermal_stress: lsm_elastic_stress_cells and lsm_elastic_stress with every normal
 *      unit stress replaced by shat_ii − t_C; in 2-D the out-of-plane one is lambda·tr − t_C for LSM_PLANE_STRAIN and stays 0 for
 *      LSM_PLANE_STRESS; the shears are unchanged; the von Mises value is the same formula on these values, so that it differs
 *      from the isothermal one in plane stress only (elsewhere t_C cancels in the three differences, up to rounding).  what:
 *      LSM_STRESS_STRESS or LSM_STRESS_VON_MISES; LSM_STRESS_STRAIN is refused: the total strain is lsm_elastic_stress's.  The node
 *      fields follow the stress recovery's rule.
 *      lsm_elastic_thermal_source: q_I = (sum over the existing cells around I, ascending, of E_C·(ab_C·tr_C(v)))/(their number),
 *      nn fp64 on the device.  m_I·q_I = d(v·b_th)/dT_I: with the elastic adjoint v (A v = b_l, zero on the fixed components) it is the
 *      source lsm_elliptic_solve takes for the heat adjoint w.
 *      lsm_elastic_thermal_sensitivity: z_C = E_C·(t_C·tr_C(v) − q_C), q_C = sum_r u_r·(sum_s K0[r,s]·v_s) in
 *      lsm_elastic_energy_mutual's order; d_I = (sum of z_C over the existing cells around I, ascending)/(their number) − minus_I, minus
 *      a dense field converted to fp64, or NULL (nothing is subtracted), rounded once into the dense field g_out.  z_C is
 *      E_C·dJ'/dE_C, exact for the discrete problem, for J' = sum b_l·u, the state A u = b_m + b_th(T) and the adjoint v, prescribed
 *      non-zero displacements included.  With minus = lsm_elliptic_energy_mutual(T, w) of the heat state and its adjoint, d is the
 *      integrand of the shape derivative of l·u in the library's convention, for the coupled problem in which one phi gives both the
 *      conductivity and the modulus.  With alpha = 0 it is −lsm_elastic_energy_mutual bit for bit (for a finite T).
 *      LSM_ERR_INVALID without running anything: a missing or repeated field (within u, within v; T one of u's or v's), an output that
 *      is missing or one of the inputs, a non-finite t_ref, a non-finite scalar alpha where it is read, a `what` not listed above.  A
 *      non-finite T, u, v or alpha cell propagates.  The calls use the object's scratch vectors as the stress recovery does (only
 *      lsm_elastic_thermal_stress writes them): none must run concurrently with a solve of the object or of its modes, and the results
 *      of a later solve are unaffected. */
int lsm_elastic_thermal_load(LsmElastic* s, const void* T, double t_ref, double alpha, const double* alpha_cells, double* f_out);
int lsm_elastic_thermal_stress_cells(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* T, double t_ref, double alpha,
                                     const double* alpha_cells, int what, double* out);
int lsm_elastic_thermal_stress(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* T, double t_ref, double alpha,
                               const double* alpha_cells, int what, void* o0, void* o1, void* o2, void* o3, void* o4, void* o5);
int lsm_elastic_thermal_source(LsmElastic* s, const void* v0, const void* v1, const void* v2, double alpha, const double* alpha_cells, double* q_out);
int lsm_elastic_thermal_sensitivity(LsmElastic* s, const void* u0, const void* u1, const void* u2, const void* v0, const void* v1, const void* v2,
                                    const void* T, double t_ref, double alpha, const double* alpha_cells, const void* minus, void* g_out);

/* ---- volume_mesh(ϕ, level): the interior {ϕ < level} as a body-fitted simplicial mesh — the splitting phase of
 *      mmg2d_O3 / mmg3d_O3 -ls that export_volume_mesh (ext/MMGVolumeExt.jl) runs over the Kuhn triangulation of the grid,
 *      without the remesher.  Every simplex of the Freudenthal subdivision (lsm_iso_*'s) that the level crosses is split at
 *      lsm_iso's cut vertices, without Steiner points: a conforming mesh of triangles (2-D) or tetrahedra
 *      (3-D) of non-negative signed volume whose boundary inside the box is exactly lsm_iso's mesh.  phi: a dense field; a
 *      band mask is refused (a band does not hold the interior); only the interior of phi is read: no ghost fill.  2-D and
 *      3-D, single device, level finite; an empty result is LSM_OK.  lsm_vol_create: counts[3] := {vertices, elements,
 *      interface elements}.  lsm_vol_read copies into device buffers (each may be NULL): vertices nv x ndim doubles
 *      (point-major), ordered by the grid node that owns them (axis 0 fastest; the node itself if inside, then the cut
 *      vertices of its edges); elements ne x (ndim + 1) int64, 0-based vertex numbers, ordered by cell; interface ni x ndim
 *      int64: lsm_iso's elements, in its order and orientation, in this mesh's vertex numbers.  Synchronous. */
typedef struct LsmVol LsmVol;
int lsm_vol_create(LsmHandle* h, const void* phi, const void* mask, double level, LsmVol** out, int64_t* counts);
int lsm_vol_read(LsmVol* s, void* vertices, void* elements, void* interface_elements);
void lsm_vol_destroy(LsmVol* s);

/* ---- render(ϕ, camera): pictures of the interface — what ext/MakieExt.jl:142-171 draws.  3-D: volume!(ϕ; algorithm = :iso,
 *      isovalue = level), the first hit of a ray march through the trilinear interpolant, shaded by its gradient; 2-D:
 *      contourf! under contour! at the level, a band's active cells tinted (tests/_render_ref.py restates
 *      every operation).  phi: a dense field (mask NULL) or a band field with its mask (a sample whose cell has a corner off
 *      the band is void: off-band values decide nothing); only the interior is read: no ghost fill.  2-D and 3-D, single
 *      device, level finite.
 *      lsm_render_create builds the table of bricks (8 cells per axis: void / outside / inside / mixed, one byte each) that
 *      lets rays step over uniform regions (3-D; nothing in 2-D) and BORROWS phi and mask: both must stay alive, and phi
 *      unchanged, between create / refresh and the last draw that follows.  lsm_render_refresh rebuilds the table after phi (or
 *      the band) changed in place.  Both are asynchronous on the handle's stream.
 *      lsm_render_draw writes one picture of width x height pixels, row 0 at the top, into device buffers (each may be NULL):
 *      rgba height x width x 4 bytes (4-byte aligned); 3-D: depth height x width doubles (distance along the unit ray, +inf
 *      where nothing is hit) and normal height x width x 3 doubles (unit gradient at the hit, pointing to ϕ increasing, 0 where
 *      nothing is hit); 2-D: cls height x width bytes (0 outside, 1 inside, 2 line, 3 void, 4 / 5 active band cell outside /
 *      inside), normal unused.  Asynchronous on `stream`.
 *      camera (3-D; may be NULL in 2-D): eye[3], forward[3] (unit), right_s[3], up_s[3], orthographic flag.  Pixel (i, j) has
 *      sx = 2(i + 1/2)/width - 1, sy = 1 - 2(j + 1/2)/height; perspective: origin eye, direction forward + sx right_s +
 *      sy up_s, normalised; orthographic (flag != 0): origin eye + sx right_s + sy up_s, direction forward.
 *      style, 3-D, 9 doubles:  [0..2] colour of the surface (0..255 each), [3..5] background, [6] ambient in 0..1, [7] step:
 *      sample spacing in units of the smallest meshsize (>= 1/1024), [8] bisections of a bracket (0..30).
 *      style, 2-D, 23 doubles: [0] line width in pixels, [1..4] extent x0, x1, y0, y1 (x1 > x0, y1 > y0; y1 is the top row),
 *      [5..22] rgb of the classes 0..5.
 *      lsm_render_bricks (synchronous): dims[3] := bricks per axis (0 in 2-D); table (device, may be NULL): one byte per brick,
 *      axis 0 fastest: bits 0..1 the state (0 void, 1 outside, 2 inside, 3 mixed), bit 2 set if rays may step over it (the
 *      brick and its 26 neighbours in the grid have the same state, not mixed). */
typedef struct LsmRender LsmRender;
int lsm_render_create(LsmHandle* h, const void* phi, const void* mask, double level, LsmRender** out);
int lsm_render_refresh(LsmRender* s);
int lsm_render_draw(LsmRender* s, const double camera[13], int width, int height, const double style[], void* rgba, void* depth_or_cls,
                    void* normal, void* stream);
int lsm_render_bricks(LsmRender* s, int64_t* dims, void* table);
void lsm_render_destroy(LsmRender* s);

/* ---- NarrowBandMeshField (src/meshfield.jl:314-588) on the device.
 *      The band is a byte mask (1 = active node) over the same padded index space as the values
 *      (allocate LsmLayout.total bytes; ghost entries stay 0).  Values stay in the dense padded array.
 *      PeriodicBC is rejected, as in the reference (:339-340).
 *
 *      lsm_band_update      update_band! (:555-588) and everything derived from the new band in one call:
 *                           cut cells of the band (or of the whole grid when from_dense != 0) seed their
 *                           corners, nlayers L1 dilations grow the new band, newly active nodes get the
 *                           affine extrapolant from the OLD band; mask is replaced; tiles := per-tile
 *                           activity flags (size: lsm_band_tile_count; tile = the stage kernel's brick
 *                           with mc planes; on entry the OLD band's flags unless from_dense); then
 *                           lsm_band_halo on the new band.  scratch_a/b: mask-sized.
 *      lsm_band_halo        halo_mask := the in-grid nodes a stencil centred on a band node reads — up to
 *                           3 nodes along each axis, the 3^N box, and the in-grid nodes out-of-grid
 *                           positions resolve to through _getindexbc (:248-260);  halo_list := one 16-byte
 *                           entry per non-band halo node naming its nearest band node
 *                           (_nearest_band_node, :513-530 — a function of the mask alone, so it is found
 *                           once per band).  halo_count: device uint32, receives the number of entries
 *                           wanted; if it exceeds halo_cap the list is truncated — repeat with a larger one.
 *      lsm_band_fill_list   _extrapolate_to_ghost (:481-511) materialised on the halo from halo_list, so that
 *                           stencils read plain entries; follow with lsm_fill_ghosts for the out-of-grid
 *                           layers.  Called on every stage input.
 *      lsm_band_prepare     lsm_band_fill_list + lsm_fill_ghosts in one call (the ghost fill is skipped while the
 *                           band stays a tile away from every face of the grid).
 *      lsm_band_fill        the same by a fresh search for targets & !band nodes; tiles = NULL visits the whole
 *                           grid (scalar getindex path).
 *      lsm_stage_band       lsm_stage restricted to band nodes (tiles without band nodes are skipped)
 *      lsm_compute_cfl_band compute_cfl over active_nodeindices (tiles/mc: optional tile flags, to step over empty tiles)
 *      lsm_band_count       number of active nodes;  lsm_band_missed: a value was requested farther than
 *                           the search radius (6) from the band since the last call (the reference throws);
 *      lsm_band_status      lsm_band_missed and *halo_count in one synchronisation.  It also brings the lengths
 *                           of the compact tile lists lsm_band_update built on the device to the host: from
 *                           then on band kernels launch one block per listed tile instead of one per tile
 *                           (without the call everything still works, over all tiles). */
int lsm_band_tile_count(LsmHandle* h, int mc, int64_t* ntiles);
int lsm_band_update(LsmHandle* h, void* vals, void* mask, int from_dense, int nlayers, void* scratch_a, void* scratch_b,
                    void* halo_mask, void* tiles, int mc, void* halo_list, int64_t halo_cap, void* halo_count);
int lsm_band_halo(LsmHandle* h, const void* vals, const void* mask, void* halo_mask, const void* tiles, int mc,
                  void* halo_list, int64_t halo_cap, void* halo_count);
int lsm_band_retile(LsmHandle* h, const void* mask, void* tiles, int mc);   /* tile flags + lists of a mask changed from outside */
/* The handle keys what it knows about a band (the compact tile lists of `tiles`, the length of halo_list as lsm_band_status
 * last read it, a prefetched dt) by the ADDRESSES of the caller's buffers.  After rewriting mask / tiles / halo_list /
 * halo_count IN PLACE (copy! of another band into the same buffers) call lsm_band_retile + lsm_band_status — which rebuild that
 * state — or at least lsm_band_invalidate, after which the band kernels run over all tiles and take the list's length from
 * the device until the next lsm_band_status.  (The gather of lsm_band_fill_list is bounded by the device counter in any case.)
 * The prefetched dt of a band obeys lsm_cfl_cache's contract: tables rewritten in place -> lsm_cfl_cache(h, 0). */
int lsm_band_invalidate(LsmHandle* h);
int lsm_band_fill_list(LsmHandle* h, void* vals, const void* mask, const void* halo_list, int64_t halo_cap,
                       const void* halo_count);
int lsm_band_prepare(LsmHandle* h, void* vals, const void* mask, const void* halo_list, int64_t halo_cap,
                     const void* halo_count, const void* tiles, int mc);
int lsm_band_fill(LsmHandle* h, void* vals, const void* mask, const void* targets, const void* tiles, int mc);
int lsm_band_count(LsmHandle* h, const void* mask, int64_t* count);
int lsm_band_missed(LsmHandle* h, int* missed);
int lsm_band_status(LsmHandle* h, const void* halo_count, int64_t* count, int* missed);
int lsm_stage_band(LsmHandle* h, const LsmTerm* terms, int nterms, const void* psi, const void* phin, void* out,
                   void* out2, int base_mode, double cdt, double cdt2, double t_stage, const void* mask,
                   const void* tiles, int mc, void* stream);
int lsm_compute_cfl_band(LsmHandle* h, const LsmTerm* terms, int nterms, const void* phi, const void* mask,
                         const void* tiles, int mc, double t, double* dt_out);

/* ---- _advance!(integrator, ϕ::NarrowBandMeshField, buffers, terms, tc, Δt): the reference steps a band with the same
 *      _advance! as a dense field (src/timestepping.jl:128-137,143-164,170-202), its node loop running over
 *      active_nodeindices (src/meshfield.jl:330-333) and its stencil reads outside the band answered by
 *      _extrapolate_to_ghost (:481-511).  Here: per stage lsm_band_prepare on the stage input, then lsm_stage_band; the
 *      integrator's combinations as in lsm_advance_*.  LsmBand names what lsm_band_update maintains for the field (all
 *      caller-owned device buffers).  phi / buf1 / buf2 are padded value arrays; their off-band entries are scratch (buffers
 *      need no initialisation).  The hook runs before each stage with the PREPARED stage input, stream synchronised.  On a
 *      slab with lsm_band_overlap_config the overlap planes of every stage result are refreshed from their owners
 *      (lsm_band_overlap_values).  Follow an accepted step with lsm_band_update (update_band!, src/timestepping.jl:115). */
typedef struct LsmBand {
    void* mask;                   /* byte mask of the active nodes (LsmLayout.total bytes) */
    void* tiles;                  /* per-tile activity flags (lsm_band_tile_count bytes) */
    int32_t mc;                   /* planes per tile along the last dimension */
    int32_t _pad;
    void* halo_list;              /* lsm_band_update / lsm_band_halo: (halo node, nearest band node) entries, 16 bytes each */
    int64_t halo_cap;
    void* halo_count;             /* device uint32 */
} LsmBand;
int lsm_advance_band_fe(LsmHandle* h, const LsmTerm* terms, int nterms, const LsmBand* band, void* phi, void* buf1,
                        double tc, double dt, LsmStageHook hook, void* user);
int lsm_advance_band_rk2(LsmHandle* h, const LsmTerm* terms, int nterms, const LsmBand* band, void* phi, void* buf1, void* buf2,
                         double tc, double dt, LsmStageHook hook, void* user);
int lsm_advance_band_rk3(LsmHandle* h, const LsmTerm* terms, int nterms, const LsmBand* band, void* phi, void* buf1, void* buf2,
                         double tc, double dt, LsmStageHook hook, void* user);

/* ---- reinitialize!(ϕ; order = 3, upsample = 2, maxiters = 20, xtol, ftol) (src/reinitializer.jl:12-42):
 *      every active node (every node when mask == NULL, the band nodes otherwise) is overwritten with
 *      sign(ϕ)·distance to the zero set of the piecewise-polynomial interpolant of ϕ (NewtonSDF, src/sdf.jl:
 *      interface samples by Newton projection, nearest sample as seed, Newton–Lagrange closest point on the
 *      seed cell's Bernstein patch).  phi: ghosts filled (lsm_fill_ghosts) and, with a mask, the band halo
 *      filled (lsm_band_prepare); work: a field-sized scratch array.  order in 1..5.
 *      Out: candidate cells sampled, nodes whose solve did not converge (the reference warns), nodes left
 *      untouched because the field has no interface sample at all.
 *      The handle keeps the call's device buffers and sizes the next call's from them: a call is enqueued whole, synchronises the
 *      stream once at its end, and repeats itself when the band has outgrown the buffers (ϕ is written by the last round only).
 *      A call that fails releases the buffers the handle keeps; the next call sizes them afresh. */
int lsm_reinitialize(LsmHandle* h, void* phi, const void* mask, void* work, int order, int upsample, int maxiters,
                     double xtol, double ftol, int64_t* ncandidate_cells, int64_t* nfail, int64_t* nfar);

/* ---- tuning switches ----
 * Every switch has the name of an environment variable.  The environment is read ONCE per process, when the first handle is
 * created; every handle starts from those values and lsm_set_tuning changes one handle's (tests and A/B measurements flip
 * them between launches).  None of them changes a result beyond what its description says; the whole GPU test suite passes
 * under each.  Unknown names are refused.  (Experiments that were measured and lost have no switch: their record is DESIGN.md.)
 * The four launch-geometry switches (LSM_STAGE_TAIL, LSM_STAGE_MC, LSM_STAGE_MC2: 0 .. 65536; LSM_STAGE_TAIL_DYN: 0 .. 1000) take
 * every value of their range — a chunk of one plane included — with the same results (tests/test_gpu_stage_geometry.py);
 * lsm_set_tuning refuses a value outside it with LSM_ERR_INVALID, and such a value in the environment leaves the default.
 *
 *   name                    default  meaning
 *   LSM_STAGE_TAIL              16   planes per chunk of the graded tail of a dense 3-D stage launch (0: no tail)
 *   LSM_STAGE_TAIL_DYN          25   % spare workgroups of the dynamic tail (0: the static tail)
 *   LSM_STAGE_MC                 0   planes per march chunk in 3-D, the pair kernels included (0: 64, shorter on small grids)
 *   LSM_STAGE_MC2                0   rows per march chunk in 2-D (0: 8)
 *   LSM_PAIRS                    1   two nodes per thread for dense single-term stages (0: one node per thread)
 *   LSM_STAGE_GENERIC            0   general stage kernels instead of the plain variants (diagnostic: same results)
 *   LSM_XREDIRECT                1   FAST steps: x / y ghosts of copy-type faces (periodic, symmetry, NeumannBC) are read from the
 *                                    node the boundary condition copies instead of being materialised (a copied -0.0 stays -0.0)
 *   LSM_MREDIRECT                1   ... and NeumannBC faces of the march (last) axis by clamping the march at the boundary plane: a FAST
 *                                    step whose other faces are served by the loads launches no ghost fill at all
 *   LSM_GHOST_FULL_DEPTH         0   ghost fills write all LSM_GHOST layers (default: the layers the step's stencils read)
 *   LSM_BAND_BRICKS              1   narrow band: the stage with one lane per band node (0: the tiled stage; bitwise equal)
 *   LSM_BAND_BITS                1   narrow band: update_band! on bit rows (0: the byte-mask kernels; bitwise equal)
 *   LSM_BAND_CFL_PREFETCH        1   narrow band: dt of the next step reduced right behind lsm_band_update
 *   LSM_BAND_BYTES               0   narrow band: byte-mask kernels in 3-D too (the path of wide bands and bands at a face)
 *   LSM_BAND_NO_LISTS            0   narrow band: launches over all tiles instead of the compact tile lists
 *   LSM_STATUS_SPIN              1   lsm_band_status spins on the status kernel's ticket in pinned memory (0: stream synchronise)
 *   LSM_SLAB_OVERLAP             1   slab steps update the interface planes first (read when a communicator is attached)
 *   LSM_COMM_TIMEOUT_MS      60000   how long a rank waits for its peers before LSM_ERR_COMM
 *   LSM_LAYOUT_ALIGN             1   rows of the padded layout start on 64-byte lines (environment only: fixed by lsm_create)
 *   LSM_RENDER_SKIP              1   lsm_render_draw: rays step over uniform bricks (0: every lattice sample is loaded; identical pictures)
 *   LSM_SEMILAG_STAGE            0   lsm_advance_semilag: the direct gather everywhere (1: workgroups whose departure box fits read the stencils
 *                                    from LDS, the others from global memory — faster for order 5, not for orders 1 and 3; 2: the same, and
 *                                    LSM_ERR_INVALID when a box does not fit; 0 .. 2, identical bits) */
int lsm_set_tuning(LsmHandle* h, const char* name, int value);
int lsm_get_tuning(const LsmHandle* h, const char* name, int* value);

/* ---- measurement: HIP-event timing of the stage kernels on the handle's stream ----
 * on = 0: off; on = 1: an event pair around every stage launch; on = N > 1: around every N-th launch (an event costs the
 * stream ≈3.7 µs on MI355X: six per RK3 step are 22 µs — 20 % of a 2048² step, 0.6 % of a 512³ one).  lsm_profile_read
 * returns the number of stage launches since the last read and their total time — with a sampling period, the mean of
 * the sampled launches times that number. */
int lsm_profile_enable(LsmHandle* h, int on);
int lsm_profile_read(LsmHandle* h, int64_t* n_stage_launches, double* stage_ms_total);   /* synchronises; resets */

#ifdef __cplusplus
}
#endif
#endif /* LSM_H */
