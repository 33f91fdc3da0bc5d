# ROCMeshField.jl — the reference-side binding a maintainer would add to LevelSetMethods.jl
# (e.g. as ext/ROCMExt.jl with AMDGPU as a weak dependency).  Host code stays Julia; AMDGPU.jl only
# owns the device arrays; every kernel is reached through `ccall` into libhiplsm.so (include/lsm.h).
#
# NEVER EXECUTED IN THIS REPOSITORY: there is no Julia runtime in the build container (SURVEY.md, "Container
# facts").  What is checked mechanically is its C side: tests/test_julia_binding.py parses this file and compares every
# struct (field order and types) and every `ccall` (symbol, return type, argument count and kinds) with include/lsm.h.
# The Python host layer (levelsetmethods.jl_amd/api.py) drives the SAME C ABI call for call and is what the GPU tests
# exercise; this file mirrors it one to one.
#
# Extension point used: the AbstractMeshField interface (src/meshfield.jl:11-33) and the methods
# the integrator reaches a field through (src/timestepping.jl:126-202, src/levelsetterms.jl:22-38).

module ROCMExt

using AMDGPU
using LevelSetMethods
import LevelSetMethods as LSM
using StaticArrays

const libhiplsm = get(ENV, "LSM_AMD_LIB", "libhiplsm.so")
const LSM_GHOST = 3
const LSM_COMM_ID_BYTES = 128

# ---- POD mirrors of include/lsm.h ------------------------------------------------------------
struct LsmGrid
    ndim::Int32
    _pad::Int32
    n::NTuple{3, Int64}
    lc::NTuple{3, Float64}
    hc::NTuple{3, Float64}
end
struct LsmBc
    kind::Int32
    degree::Int32
end
struct LsmSlab
    lo::Int64
    n::Int64
end
struct LsmLayout
    n::NTuple{3, Int64}
    g::NTuple{3, Int64}
    stride::NTuple{3, Int64}
    origin::Int64
    total::Int64
end
struct LsmCoeff
    kind::Int32
    time_kind::Int32
    time_param::Float64
    value::NTuple{4, Float64}
    field::NTuple{3, Ptr{Cvoid}}
    sep::NTuple{3, Ptr{Float64}}
end
struct LsmTerm
    kind::Int32
    scheme::Int32
    coeff::LsmCoeff
    s0::Ptr{Cvoid}
end

_pad3(t, fill) = ntuple(i -> i <= length(t) ? t[i] : fill, 3)
_pad4(t) = ntuple(i -> i <= length(t) ? t[i] : 0.0, 4)

lsmgrid(g::LSM.CartesianGrid{N}) where {N} =
    LsmGrid(N, 0, _pad3(Int64.(g.n), Int64(1)), _pad3(Float64.(g.lc), 0.0), _pad3(Float64.(g.hc), 1.0))

lsmbc(::LSM.PeriodicBC) = LsmBc(0, 0)
lsmbc(::LSM.ExtrapolationBC{P}) where {P} = LsmBc(1, P)
lsmbc(::LSM.SymmetryBC) = LsmBc(2, 0)
const LSM_BC_NONE = LsmBc(3, 0)          # slab interface: ghosts come from the halo exchange

function _check(h, code, what)
    code == 0 && return
    msg = unsafe_string(ccall((:lsm_last_error, libhiplsm), Cstring, (Ptr{Cvoid},), h))
    error("$what failed ($code): $msg")
end

# ---- the handle: one per (mesh, bc, slab, storage type), shared by a field and its copies ----------------
mutable struct Handle
    ptr::Ptr{Cvoid}
    layout::LsmLayout
    strict::Bool
    lo::Int          # first plane (0-based) of the slab along the last dimension; 0 on a whole grid
    rank::Int
    world::Int
end

_dtype(::Type{Float64}) = Cint(0)       # LSM_DTYPE_F64
_dtype(::Type{Float32}) = Cint(1)       # LSM_DTYPE_F32: a storage format, every computation is Float64 (include/lsm.h)

# slab = nothing (whole grid) or (lo, n, rank, world): planes lo+1:lo+n of the last dimension (SURVEY.md §8e)
function Handle(mesh::LSM.CartesianGrid{N}, bcs, ::Type{S}; strict = false, slab = nothing) where {N, S}
    g = Ref(lsmgrid(mesh))
    bc = [d <= N ? lsmbc(bcs[d][s]) : LsmBc(1, 0) for s in 1:2, d in 1:3]   # C order bc[dim][side]
    lo, rank, world = 0, 0, 1
    slabref = C_NULL
    sl = Ref(LsmSlab(0, mesh.n[N]))
    if slab !== nothing
        lo, n, rank, world = slab
        periodic = bcs[N][1] isa LSM.PeriodicBC
        (rank > 0 || (periodic && world > 1)) && (bc[1, N] = LSM_BC_NONE)          # faces towards neighbouring ranks;
        (rank < world - 1 || (periodic && world > 1)) && (bc[2, N] = LSM_BC_NONE)  # both on a periodic ring
        sl[] = LsmSlab(lo, n)
        slabref = Base.unsafe_convert(Ptr{LsmSlab}, sl)
    end
    h = Ref{Ptr{Cvoid}}(C_NULL)
    code = GC.@preserve sl ccall((:lsm_create, libhiplsm), Cint,
        (Ref{LsmGrid}, Ptr{LsmBc}, Ptr{LsmSlab}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
        g, bc, slabref, _dtype(S), strict ? 1 : 0, AMDGPU.device_id(AMDGPU.device()) - 1, h)
    _check(C_NULL, code, "lsm_create")
    # kernels run on the stream AMDGPU.jl uses for its own copies
    _check(h[], ccall((:lsm_set_stream, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h[], AMDGPU.stream().stream), "lsm_set_stream")
    lay = Ref{LsmLayout}()
    _check(h[], ccall((:lsm_layout, libhiplsm), Cint, (Ptr{Cvoid}, Ref{LsmLayout}), h[], lay), "lsm_layout")
    hd = Handle(h[], lay[], strict, lo, rank, world)
    finalizer(x -> ccall((:lsm_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), x.ptr), hd)   # lsm_destroy detaches a communicator
    return hd
end

# ---- the device field --------------------------------------------------------------------------
"""
    ROCMeshField{N,T,B,S} <: AbstractMeshField{N,T,S}

Dense level-set field resident in HBM in libhiplsm's padded layout (ghost layers materialised).
`S` is the storage type: `Float64`, or `Float32` (LSM_DTYPE_F32 handles: values widen exactly on load,
every computation is Float64, results are rounded once on store).
"""
mutable struct ROCMeshField{N, T, B, S} <: LSM.AbstractMeshField{N, T, S}
    buf::ROCVector{S}
    mesh::LSM.CartesianGrid{N, T}
    bcs::B
    h::Handle
    samples::Dict{UInt, Vector{ROCVector{Float64}}}   # closures sampled on the host into FIELD coefficients (see _coeff)
end

_local(v::AbstractArray{<:Any, N}, slab) where {N} = slab === nothing ? v : collect(selectdim(v, N, (slab[1] + 1):(slab[1] + slab[2])))

function ROCMeshField(ϕ::LSM.MeshField{N, T}; strict = false, slab = nothing) where {N, T}
    LSM._check_bc(ϕ)
    S = eltype(values(ϕ))
    bcs = LSM.boundary_conditions(ϕ)
    h = Handle(LSM.mesh(ϕ), bcs, S; strict, slab)
    buf = AMDGPU.zeros(S, h.layout.total)
    f = ROCMeshField{N, T, typeof(bcs), S}(buf, LSM.mesh(ϕ), bcs, h, Dict{UInt, Vector{ROCVector{Float64}}}())
    host = _local(values(ϕ), slab)
    _check(h.ptr, ccall((:lsm_upload, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h.ptr, pointer(buf), host), "lsm_upload")
    return check_range(f)
end

# values(ϕ): host copy of the (local) interior on demand (show, hooks, tests)
function Base.values(ϕ::ROCMeshField{N, T, B, S}) where {N, T, B, S}
    out = Array{S, N}(undef, ntuple(d -> Int(ϕ.h.layout.n[d]), N))
    _check(ϕ.h.ptr, ccall((:lsm_download, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ϕ.h.ptr, pointer(ϕ.buf), out), "lsm_download")
    return out
end
LSM.MeshField(ϕ::ROCMeshField) = LSM.MeshField(values(ϕ), LSM.mesh(ϕ), ϕ.bcs)

# a copy shares the handle (same mesh, bc, slab, storage type, mode and communicator): only the values are new
Base.copy(ϕ::ROCMeshField{N, T, B, S}) where {N, T, B, S} = ROCMeshField{N, T, B, S}(copy(ϕ.buf), ϕ.mesh, ϕ.bcs, ϕ.h, ϕ.samples)
Base.copy!(dst::ROCMeshField, src::ROCMeshField) = (copyto!(dst.buf, src.buf); dst)
LSM.update_band!(::ROCMeshField) = nothing
# scalar indexing: slow path for tests and hooks
Base.getindex(ϕ::ROCMeshField, I::CartesianIndex) = LSM.MeshField(ϕ)[I]

# ---- multi-GPU: one process per GPU, one slab per process (include/lsm.h, "multi-GPU") -----------------------
# rank 0:  id = comm_unique_id();  hand `id` to every rank (MPI.Bcast!, a file, ...)
# each:    ϕ = ROCMeshField(ϕ_host; slab = (lo, n, rank, world));  attach_rccl!(ϕ, id)
# integrate!(eq, tf) then runs unchanged: _advance! -> lsm_advance_* exchanges the ghost planes after every stage
# (overlapped with the interior update), compute_cfl all-reduces Δt.
function comm_unique_id()
    id = Vector{UInt8}(undef, LSM_COMM_ID_BYTES)
    _check(C_NULL, ccall((:lsm_comm_unique_id, libhiplsm), Cint, (Ptr{Cvoid},), id), "lsm_comm_unique_id")
    return id
end
function attach_rccl!(ϕ::ROCMeshField, id::Vector{UInt8})
    _check(ϕ.h.ptr, ccall((:lsm_comm_attach_rccl, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint), ϕ.h.ptr, id, ϕ.h.rank, ϕ.h.world), "lsm_comm_attach_rccl")
    halo!(ϕ)
    return ϕ
end
# every rank as a field of THIS process (one Julia task per rank, or one task driving all ranks stage by stage)
function attach_local!(ϕs::Vector{<:ROCMeshField})
    hs = Ptr{Cvoid}[ϕ.h.ptr for ϕ in ϕs]
    _check(hs[1], ccall((:lsm_comm_attach_local, libhiplsm), Cint, (Ptr{Ptr{Cvoid}}, Cint), hs, length(hs)), "lsm_comm_attach_local")
    return ϕs
end
# ghosts of a field written from outside a step: boundary conditions, then the neighbours' planes
function halo!(ϕ::ROCMeshField)
    _check(ϕ.h.ptr, ccall((:lsm_fill_ghosts, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}), ϕ.h.ptr, pointer(ϕ.buf), 7, C_NULL), "lsm_fill_ghosts")
    ϕ.h.world > 1 && _check(ϕ.h.ptr, ccall((:lsm_halo_exchange, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ϕ.h.ptr, pointer(ϕ.buf)), "lsm_halo_exchange")
    return ϕ
end
# the two halves, for a driver that overlaps the exchange itself (lsm_stage_planes on the interface planes, start, interior, wait)
halo_start!(ϕ::ROCMeshField) = _check(ϕ.h.ptr, ccall((:lsm_halo_start, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ϕ.h.ptr, pointer(ϕ.buf)), "lsm_halo_start")
halo_wait!(ϕ::ROCMeshField) = _check(ϕ.h.ptr, ccall((:lsm_halo_wait, libhiplsm), Cint, (Ptr{Cvoid},), ϕ.h.ptr), "lsm_halo_wait")
set_overlap!(ϕ::ROCMeshField, on::Bool) = _check(ϕ.h.ptr, ccall((:lsm_comm_set_overlap, libhiplsm), Cint, (Ptr{Cvoid}, Cint), ϕ.h.ptr, on), "lsm_comm_set_overlap")
detach!(ϕ::ROCMeshField) = _check(ϕ.h.ptr, ccall((:lsm_comm_detach, libhiplsm), Cint, (Ptr{Cvoid},), ϕ.h.ptr), "lsm_comm_detach")
function comm_info(ϕ::ROCMeshField)
    r, w, t = Ref{Cint}(), Ref{Cint}(), Ref{Cint}()
    _check(ϕ.h.ptr, ccall((:lsm_comm_info, libhiplsm), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}), ϕ.h.ptr, r, w, t), "lsm_comm_info")
    return (rank = Int(r[]), world = Int(w[]), transport = Int(t[]))
end

# ---- terms -> LsmTerm ---------------------------------------------------------------------------
# Julia closures cannot run on the device (src/levelsetterms.jl:42-43 evaluates `f(getnode(ϕ, I), t)` per node):
# constants, catalogued analytic fields and device fields are passed through; a closure is sampled on the host into a
# FIELD coefficient — at construction of the LsmTerm and again, by the stage hook, before every stage at its stage time.
struct RigidRotation; ω::Float64; c::NTuple{2, Float64}; end     # u = ω·(-(x₂-c₂), x₁-c₁, 0)

const _NOFIELD = (C_NULL, C_NULL, C_NULL)
const _NOSEP = (Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL))
_coeff(v::Number, ϕ, t, K) = LsmCoeff(0, 0, 1.0, (Float64(v), 0.0, 0.0, 0.0), _NOFIELD, _NOSEP)
_coeff(v::Union{SVector, Tuple{Vararg{Number}}}, ϕ, t, K) = LsmCoeff(0, 0, 1.0, _pad4(Float64.(Tuple(v))), _NOFIELD, _NOSEP)
_coeff(r::RigidRotation, ϕ, t, K) = LsmCoeff(1, 0, 1.0, (r.ω, r.c[1], r.c[2], 0.0), _NOFIELD, _NOSEP)
# device fields: the library reads coefficient fields as Float64 side arrays in ϕ's padded layout
_f64(f::ROCMeshField{N, T, B, Float64}, ϕ) where {N, T, B} = f.buf
_f64(f::ROCMeshField, ϕ) = get!(() -> [ROCVector{Float64}(undef, length(f.buf))], ϕ.samples, objectid(f))[1] .= f.buf   # a Float32 field widens exactly
_coeff(f::ROCMeshField, ϕ, t, K) = LsmCoeff(3, 0, 1.0, (0.0, 0.0, 0.0, 0.0), (Ptr{Cvoid}(pointer(_f64(f, ϕ))), C_NULL, C_NULL), _NOSEP)
_coeff(fs::Tuple{Vararg{ROCMeshField}}, ϕ, t, K) =
    LsmCoeff(3, 0, 1.0, (0.0, 0.0, 0.0, 0.0), _pad3(map(f -> Ptr{Cvoid}(pointer(_f64(f, ϕ))), fs), C_NULL), _NOSEP)
# a closure f(x, t) -> Number | SVector: K components sampled at the local nodes, uploaded into arrays that live as long as ϕ's handle
function _coeff(f::Function, ϕ, t, K)      # ϕ::ROCField (dense or band: both carry mesh, h, samples)
    N = length(ϕ.mesh.n)
    arrs = get!(() -> [AMDGPU.zeros(Float64, ϕ.h.layout.total) for _ in 1:K], ϕ.samples, objectid(f))
    nloc = ntuple(d -> Int(ϕ.h.layout.n[d]), N)
    off = ntuple(d -> d == N ? ϕ.h.lo : 0, N)                   # a slab's nodes sit at global indices lo+1 : lo+n
    host = [Array{Float64, N}(undef, nloc) for _ in 1:K]
    for I in CartesianIndices(nloc)
        v = f(LSM.getnode(LSM.mesh(ϕ), I + CartesianIndex(off)), t)
        for k in 1:K
            host[k][I] = v[k]          # a Number indexes as v[1]
        end
    end
    for k in 1:K
        _check(ϕ.h.ptr, ccall((:lsm_upload_f64, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ϕ.h.ptr, pointer(arrs[k]), host[k]), "lsm_upload_f64")
    end
    return LsmCoeff(3, 0, 1.0, (0.0, 0.0, 0.0, 0.0), _pad3(map(a -> Ptr{Cvoid}(pointer(a)), Tuple(arrs)), C_NULL), _NOSEP)
end
_needs_sampling(c) = c isa Function

_term(t::LSM.AdvectionTerm, ϕ, tt) = LsmTerm(0, LSM.scheme(t) isa LSM.WENO5 ? 1 : 0, _coeff(LSM.velocity(t), ϕ, tt, length(ϕ.mesh.n)), C_NULL)
_term(t::LSM.NormalMotionTerm, ϕ, tt) = LsmTerm(1, 0, _coeff(LSM.speed(t), ϕ, tt, 1), C_NULL)
_term(t::LSM.CurvatureTerm, ϕ, tt) = LsmTerm(2, 0, _coeff(LSM.coefficient(t), ϕ, tt, 1), C_NULL)
_term(t::LSM.EikonalReinitializationTerm{Nothing}, ϕ, tt) = LsmTerm(3, 0, _coeff(0.0, ϕ, tt, 1), C_NULL)
_term(t::LSM.EikonalReinitializationTerm{<:ROCVector{Float64}}, ϕ, tt) = LsmTerm(3, 0, _coeff(0.0, ϕ, tt, 1), Ptr{Cvoid}(pointer(t.S₀)))
_coefficient(t::LSM.AdvectionTerm) = LSM.velocity(t)
_coefficient(t::LSM.NormalMotionTerm) = LSM.speed(t)
_coefficient(t::LSM.CurvatureTerm) = LSM.coefficient(t)
_coefficient(::LSM.EikonalReinitializationTerm) = nothing

# EikonalReinitializationTerm(ϕ₀::ROCMeshField): S₀ = ϕ₀/√(ϕ₀²+Δx²) on the device (src/levelsetterms.jl:217-221), a Float64 side array
function LSM.EikonalReinitializationTerm(ϕ₀::ROCMeshField)
    S₀ = ROCVector{Float64}(undef, length(ϕ₀.buf))
    _check(ϕ₀.h.ptr, ccall((:lsm_eikonal_sign, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ₀.h.ptr, pointer(ϕ₀.buf), pointer(S₀), C_NULL), "lsm_eikonal_sign")
    return LSM.EikonalReinitializationTerm{typeof(S₀)}(S₀)
end

# ---- the methods the integrator dispatches on -----------------------------------------------------
# compute_cfl (src/levelsetterms.jl:22-28): the library returns the raw local minimum; across slabs it is min-reduced
# with NaN winning; Julia throws.
function LSM.compute_cfl(terms, ϕ::ROCMeshField, t)
    ts = [_term(term, ϕ, t) for term in terms]
    dt = Ref{Float64}(0.0)
    _check(ϕ.h.ptr, ccall((:lsm_compute_cfl, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ptr{Cvoid}, Float64, Ref{Float64}),
        ϕ.h.ptr, ts, length(ts), pointer(ϕ.buf), t, dt), "lsm_compute_cfl")
    ϕ.h.world > 1 && _check(ϕ.h.ptr, ccall((:lsm_allreduce_dt, libhiplsm), Cint, (Ptr{Cvoid}, Ref{Float64}), ϕ.h.ptr, dt), "lsm_allreduce_dt")
    Δt = dt[]
    Δt > 0 || throw(ArgumentError("invalid time-step based on CFL condition: Δt = $Δt (check for NaN/Inf in velocity or speed)"))
    return Δt
end

# stage hook: lets update_func(field, stage_field, stage_time) run — and closure coefficients be re-sampled at the stage
# time — between stage launches (src/timestepping.jl:131,149,158,174,185,196).  NULL when every term has the default no-op
# update_func (src/levelsetterms.jl:63,141,146: `(_...) -> nothing`, one anonymous function per constructor) and no closure.
const _NOOPS = (typeof(LSM.AdvectionTerm(0).update_func), typeof(LSM.NormalMotionTerm(0).update_func))
_is_noop(t) = !hasproperty(t, :update_func) || typeof(t.update_func) in _NOOPS
function _hook(terms, fields)
    all(_is_noop, terms) && !any(t -> _needs_sampling(_coefficient(t)), terms) && return C_NULL
    cb = (user, stage, ptr, tstage) -> begin
        ψ = fields[stage + 1]
        for term in terms
            LSM.update_term!(term, ψ, tstage)
            _needs_sampling(_coefficient(term)) && _term(term, ψ, tstage)     # refresh the sampled arrays in place
        end
        Cint(0)
    end
    return @cfunction($cb, Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Float64))
end

# SemiImplicitI2OE (src/timestepping.jl:207-244): the step loop of the reference with the global solve on the device
# (lsm_advance_i2oe: matrix-free BiCGSTAB to ‖r‖₂ ≤ 1e-13‖rhs‖₂ instead of the sparse direct solve).  The reference's checks
# come first and throw its ArgumentErrors; a solve that breaks down or runs out of iterations is an ErrorException.
function LSM._integrate!(ls, ϕ::ROCMeshField, integrator::LSM.SemiImplicitI2OE, terms, tc, tf, Δt_max, prehook, posthook;
                         rtol = 1.0e-13, max_iters = 500)
    LSM._validate_i2oe_setup(ϕ, terms)
    ϕ.h.world > 1 && throw(ArgumentError("SemiImplicitI2OE runs on a single device: a slab decomposition is not supported"))
    for d in 1:length(ϕ.bcs), bc in ϕ.bcs[d]
        bc isa Union{LSM.PeriodicBC, LSM.ExtrapolationBC{0}, LSM.ExtrapolationBC{1}} ||
            error("boundary condition $bc is not supported by SemiImplicitI2OE")
    end
    term = only(terms)
    α = LSM.cfl(integrator)
    while tc <= tf - eps(tc)
        prehook(ls)
        LSM.update_term!(term, ϕ, tc)
        Δt = min(Δt_max, α * LSM.compute_cfl(terms, ϕ, tc), tf - tc)
        ts = [_term(term, ϕ, tc)]
        iters, res = Ref{Cint}(0), Ref{Float64}(0.0)
        code = ccall((:lsm_advance_i2oe, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{LsmTerm}, Ptr{Cvoid}, Float64, Float64, Float64, Cint, Ref{Cint}, Ref{Float64}),
            ϕ.h.ptr, ts, pointer(ϕ.buf), tc, Δt, rtol, max_iters, iters, res)
        _check(ϕ.h.ptr, code, "lsm_advance_i2oe")
        tc += Δt
        ls.t = tc
        posthook(ls)
    end
    ls.t = tf
    return nothing
end

# SemiLagrangian (DESIGN.md §7.30; not in the reference): large advection steps by backward characteristics, one gather pass per
# step on the device (lsm_advance_semilag).  It runs through the reference's generic step loop: one buffer, one out-of-place step,
# and the buffers of ϕ and dst change places (nothing on the handle keeps ϕ's pointer between calls).
Base.@kwdef struct SemiLagrangian <: LSM.TimeIntegrator
    cfl::Float64 = 4.0
    order::Int = 3        # degree of the Lagrange interpolant: 1, 3 or 5
    trace::Int = 2        # 1: Euler, 2: midpoint
    limiter::Bool = true  # clamp to the departure cell's extrema (Bermejo–Staniforth)
end
LSM._describe(::SemiLagrangian) = "SemiLagrangian (backward characteristics, Lagrange interpolation)"
LSM._alloc_buffers(::SemiLagrangian, ϕ::ROCMeshField) = (copy(ϕ),)
function LSM._advance!(s::SemiLagrangian, ϕ::ROCMeshField, (dst,), terms, tc, Δt)
    length(terms) == 1 && only(terms) isa LSM.AdvectionTerm || throw(ArgumentError("SemiLagrangian requires exactly one AdvectionTerm"))
    ϕ.h.world > 1 && throw(ArgumentError("SemiLagrangian runs on a single device: a slab decomposition is not supported"))
    s.order in (1, 3, 5) || throw(ArgumentError("SemiLagrangian: order must be 1, 3 or 5, got $(s.order)"))
    s.trace in (1, 2) || throw(ArgumentError("SemiLagrangian: trace must be 1 or 2, got $(s.trace)"))
    ts = [_term(only(terms), ϕ, tc)]
    _check(ϕ.h.ptr, ccall((:lsm_advance_semilag, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Cint, Cint, Cint, Ptr{Int64}),
        ϕ.h.ptr, ts, pointer(ϕ.buf), pointer(dst.buf), tc, Δt, s.order, s.trace, s.limiter ? 1 : 0, C_NULL), "lsm_advance_semilag")
    ϕ.buf, dst.buf = dst.buf, ϕ.buf
    return ϕ
end

LSM._alloc_buffers(::LSM.ForwardEuler, ϕ::ROCMeshField) = (copy(ϕ),)
LSM._alloc_buffers(::Union{LSM.RK2, LSM.RK3}, ϕ::ROCMeshField) = (copy(ϕ), copy(ϕ))

# On a slab handle with a communicator attached the same three calls run the slab's step: interface planes first, ghost
# planes exchanged over RCCL while the interior is updated (include/lsm.h).
function LSM._advance!(::LSM.ForwardEuler, ϕ::ROCMeshField, (dst,), terms, tc, Δt)
    ts = [_term(term, ϕ, tc) for term in terms]
    hook = _hook(terms, (ϕ,))
    GC.@preserve hook _check(ϕ.h.ptr, ccall((:lsm_advance_fe, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, ts, length(ts), pointer(ϕ.buf), pointer(dst.buf), tc, Δt, hook, C_NULL), "lsm_advance_fe")
    return ϕ
end
function LSM._advance!(::LSM.RK2, ϕ::ROCMeshField, (pred, corr), terms, tc, Δt)
    ts = [_term(term, ϕ, tc) for term in terms]
    hook = _hook(terms, (ϕ, pred))
    GC.@preserve hook _check(ϕ.h.ptr, ccall((:lsm_advance_rk2, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, ts, length(ts), pointer(ϕ.buf), pointer(pred.buf), pointer(corr.buf), tc, Δt, hook, C_NULL), "lsm_advance_rk2")
    return ϕ
end
function LSM._advance!(::LSM.RK3, ϕ::ROCMeshField, (buf1, buf2), terms, tc, Δt)
    ts = [_term(term, ϕ, tc) for term in terms]
    hook = _hook(terms, (ϕ, buf1, buf2))
    GC.@preserve hook _check(ϕ.h.ptr, ccall((:lsm_advance_rk3, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, ts, length(ts), pointer(ϕ.buf), pointer(buf1.buf), pointer(buf2.buf), tc, Δt, hook, C_NULL), "lsm_advance_rk3")
    return ϕ
end

# domain of the FAST arithmetic mode (include/lsm.h, LSM_FAST_MAX_ABS): called when a field is handed to an equation
function check_range(ϕ::ROCMeshField)
    ok, m = Ref{Cint}(), Ref{Float64}()
    _check(ϕ.h.ptr, ccall((:lsm_check_range, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Cint}, Ref{Float64}), ϕ.h.ptr, pointer(ϕ.buf), ok, m), "lsm_check_range")
    ok[] != 0 || throw(ArgumentError("max|ϕ| = $(m[]) is outside the domain of the FAST arithmetic mode; rescale the field or use ROCMeshField(ϕ; strict = true)"))
    return ϕ
end

# show needs extrema (src/meshfield.jl:300-303)
function Base.extrema(ϕ::ROCMeshField)
    lo, hi = Ref{Float64}(), Ref{Float64}()
    _check(ϕ.h.ptr, ccall((:lsm_extrema, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), ϕ.h.ptr, pointer(ϕ.buf), lo, hi), "lsm_extrema")
    return lo[], hi[]
end

# ---- next rows (SURVEY.md §8f) ------------------------------------------------------------------

# volume / perimeter (src/levelsetops.jl:139-149,171-183) of the local slab (sum over the ranks for a decomposed grid)
function LSM.volume(ϕ::ROCMeshField)
    out = Ref{Float64}()
    _check(ϕ.h.ptr, ccall((:lsm_volume, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}), ϕ.h.ptr, pointer(ϕ.buf), out), "lsm_volume")
    return out[]
end
function LSM.perimeter(ϕ::ROCMeshField)
    out = Ref{Float64}()
    _check(ϕ.h.ptr, ccall((:lsm_perimeter, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}), ϕ.h.ptr, pointer(ϕ.buf), out), "lsm_perimeter")
    return out[]
end

# volume / perimeter of a band field (src/levelsetops.jl:34-116,150-166); `mask` is the band's byte mask, ϕ prepared
# (lsm_band_prepare) for the perimeter's centred gradient
function band_volume(ϕ::ROCMeshField, mask::ROCVector{UInt8})
    out = Ref{Float64}()
    _check(ϕ.h.ptr, ccall((:lsm_band_volume, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}), ϕ.h.ptr, pointer(ϕ.buf), pointer(mask), out), "lsm_band_volume")
    return out[]
end
function band_perimeter(ϕ::ROCMeshField, mask::ROCVector{UInt8})
    out = Ref{Float64}()
    _check(ϕ.h.ptr, ccall((:lsm_band_perimeter, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}), ϕ.h.ptr, pointer(ϕ.buf), pointer(mask), out), "lsm_band_perimeter")
    return out[]
end

# extend_along_normals!(F, ϕ; ...) (src/velocityextension.jl:20-116); frozen = nothing -> band rule
function LSM.extend_along_normals!(F::ROCMeshField, ϕ::ROCMeshField; nb_iters = 50, cfl = 0.45, frozen = nothing,
                                   interface_band = 1.5, min_norm = 1.0e-14)
    N = length(ϕ.mesh.n)
    work = [similar(ϕ.buf) for _ in 1:(N + 1)]
    w = [i <= length(work) ? pointer(work[i]) : C_NULL for i in 1:4]
    _check(ϕ.h.ptr, ccall((:lsm_extend_along_normals, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Float64, Float64),
        ϕ.h.ptr, pointer(F.buf), pointer(ϕ.buf), frozen === nothing ? C_NULL : pointer(frozen), w[1], w[2], w[3], w[4],
        nb_iters, cfl, interface_band, min_norm), "lsm_extend_along_normals")
    _check(ϕ.h.ptr, ccall((:lsm_sync, libhiplsm), Cint, (Ptr{Cvoid},), ϕ.h.ptr), "lsm_sync")   # work buffers die here
    return F
end

# curvature / gradient / normal of ϕ at every node (src/levelsetops.jl:197-226) into Float64 device arrays in ϕ's padded
# layout; `band`: only |ϕ[I]| <= band is evaluated (else `fill`) and `frozen` marks those nodes with 1.0 — the seed loop of
# the reference's speed update functions (test/test-velocityextension.jl:118-131) without a host pass.
function curvature_field!(out::ROCVector{Float64}, ϕ::ROCMeshField; scale = 1.0, band = -1.0, fill = 0.0, frozen = nothing)
    _check(ϕ.h.ptr, ccall((:lsm_geometry, libhiplsm), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, 0, pointer(ϕ.buf), scale, band, fill, pointer(out), C_NULL, C_NULL, frozen === nothing ? C_NULL : pointer(frozen), C_NULL),
        "lsm_geometry")
    return out
end
function _vector_field!(what::Integer, outs::NTuple{N, ROCVector{Float64}}, ϕ::ROCMeshField; scale = 1.0) where {N}
    o = ntuple(d -> d <= N ? pointer(outs[d]) : C_NULL, 3)
    _check(ϕ.h.ptr, ccall((:lsm_geometry, libhiplsm), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, what, pointer(ϕ.buf), scale, -1.0, 0.0, o[1], o[2], o[3], C_NULL, C_NULL), "lsm_geometry")
    return outs
end
# band fields: the same over the active nodes of a prepared band (`mask` = the band's byte mask)
function band_curvature_field!(out::ROCVector{Float64}, ϕ::ROCMeshField, mask::ROCVector{UInt8}; scale = 1.0, band = -1.0, fill = 0.0, frozen = nothing)
    _check(ϕ.h.ptr, ccall((:lsm_band_geometry, libhiplsm), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, 0, pointer(ϕ.buf), pointer(mask), scale, band, fill, pointer(out), C_NULL, C_NULL, frozen === nothing ? C_NULL : pointer(frozen), C_NULL),
        "lsm_band_geometry")
    return out
end
gradient_field!(outs, ϕ::ROCMeshField; kw...) = _vector_field!(1, outs, ϕ; kw...)
normal_field!(outs, ϕ::ROCMeshField; kw...) = _vector_field!(2, outs, ϕ; kw...)

# InterpolatedField(ϕ, order) evaluated at points (src/interpolation.jl:117-151,228-260): `pts` is an ndim x npts device matrix
# (column = point); returns values, and fills `grad` (ndim x npts) / `hess` (ndim x ndim x npts) when given
function interpolate!(val::ROCVector{Float64}, ϕ::ROCMeshField, order::Integer, pts::ROCMatrix{Float64}; grad = nothing, hess = nothing)
    _check(ϕ.h.ptr, ccall((:lsm_interpolate, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, pointer(ϕ.buf), order, size(pts, 2), pointer(pts), pointer(val), grad === nothing ? C_NULL : pointer(grad),
        hess === nothing ? C_NULL : pointer(hess), C_NULL), "lsm_interpolate")
    return val
end

# NewtonSDF(ϕ; ...) (src/sdf.jl:57-127) as a device object: build once, query points, read the samples back
mutable struct ROCNewtonSDF
    ptr::Ptr{Cvoid}
    h::Handle
    nsamples::Int64
end
function ROCNewtonSDF(ϕ::ROCMeshField; order = 3, upsample = 2, maxiters = 10, xtol = nothing, ftol = nothing, mask = nothing)
    xt, ft = something(xtol, sqrt(eps(Float64))), something(ftol, sqrt(eps(Float64)))
    out, ns = Ref{Ptr{Cvoid}}(), Ref{Int64}()
    _check(ϕ.h.ptr, ccall((:lsm_sdf_create, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Float64, Float64, Ref{Ptr{Cvoid}}, Ref{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), mask === nothing ? C_NULL : pointer(mask), order, upsample, maxiters, xt, ft, out, ns), "lsm_sdf_create")
    sdf = ROCNewtonSDF(out[], ϕ.h, ns[])
    finalizer(s -> ccall((:lsm_sdf_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), s.ptr), sdf)
    return sdf
end
# signed distances at the columns of `pts` (ndim x npts device matrix); `cp` optionally receives the closest points
function (sdf::ROCNewtonSDF)(dist::ROCVector{Float64}, pts::ROCMatrix{Float64}; cp = nothing)
    nfail = Ref{Int64}()
    _check(sdf.h.ptr, ccall((:lsm_sdf_eval, libhiplsm), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}),
        sdf.ptr, size(pts, 2), pointer(pts), pointer(dist), cp === nothing ? C_NULL : pointer(cp), nfail), "lsm_sdf_eval")
    return dist
end
function sample_points(sdf::ROCNewtonSDF, ndim::Integer)
    out = ROCMatrix{Float64}(undef, ndim, sdf.nsamples)
    _check(sdf.h.ptr, ccall((:lsm_sdf_samples, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), sdf.ptr, pointer(out)), "lsm_sdf_samples")
    return out
end

# quadrature(ϕ; interpolation_order, quadrature_order, surface) (src/LevelSetMethods.jl:103-126, ext/ImplicitIntegrationExt.jl):
# the device arrays of the result.  cells / full_cells are 0-based linear cell indices (axis 1 fastest); the nodes of cut cell i
# (1-based) are the columns offsets[i]+1 : offsets[i+1] of coords (ndim x nodes).  rule_coords / rule_weights: the tensor rule of
# a full cell on the unit cell.  INTEGRATION.md shows how an ImplicitIntegration-aware extension wraps them into the Dict.
function quadrature_arrays(ϕ::ROCMeshField; interpolation_order, quadrature_order, surface = false, mask = nothing)
    out, c = Ref{Ptr{Cvoid}}(), zeros(Int64, 4)
    _check(ϕ.h.ptr, ccall((:lsm_quad_create, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), mask === nothing ? C_NULL : pointer(mask), interpolation_order, quadrature_order, surface, out, c), "lsm_quad_create")
    q = out[]
    try
        ncut, nnodes, nfull, nfallback = c
        N, m = ndims(ϕ), quadrature_order^ndims(ϕ)
        cells, offsets, full = ROCVector{Int64}(undef, ncut), ROCVector{Int64}(undef, ncut + 1), ROCVector{Int64}(undef, nfull)
        coords, weights = ROCMatrix{Float64}(undef, N, nnodes), ROCVector{Float64}(undef, nnodes)
        rule_coords, rule_weights = ROCMatrix{Float64}(undef, N, m), ROCVector{Float64}(undef, m)
        _check(ϕ.h.ptr, ccall((:lsm_quad_read, libhiplsm), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            q, pointer(cells), pointer(offsets), pointer(coords), pointer(weights), pointer(full), pointer(rule_coords), pointer(rule_weights)),
            "lsm_quad_read")
        total = Ref{Float64}()
        _check(ϕ.h.ptr, ccall((:lsm_quad_total, libhiplsm), Cint, (Ptr{Cvoid}, Ref{Float64}), q, total), "lsm_quad_total")
        nfallback > 0 && @warn "quadrature: $nfallback boxes reached the subdivision limit and got the low-order rule"
        return (; cells, offsets, coords, weights, full_cells = full, rule_coords, rule_weights, total = total[], nfallback)
    finally
        ccall((:lsm_quad_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), q)
    end
end

# isosurface: the interface {ϕ = level} as an indexed mesh (include/lsm.h, lsm_iso_*): vertices ndim x nv, elements ndim x ne
# with 0-based vertex numbers (segments in 2-D, triangles in 3-D), both on the device.  `mask`: a band field's byte mask.
function isosurface_arrays(ϕ::ROCMeshField; level = 0.0, mask = nothing)
    out, c = Ref{Ptr{Cvoid}}(), zeros(Int64, 2)
    _check(ϕ.h.ptr, ccall((:lsm_iso_create, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ref{Ptr{Cvoid}}, Ptr{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), mask === nothing ? C_NULL : pointer(mask), level, out, c), "lsm_iso_create")
    s = out[]
    try
        nv, ne = c
        vertices, elements = ROCMatrix{Float64}(undef, ndims(ϕ), nv), ROCMatrix{Int64}(undef, ndims(ϕ), ne)
        _check(ϕ.h.ptr, ccall((:lsm_iso_read, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), s, pointer(vertices), pointer(elements)), "lsm_iso_read")
        return (; vertices, elements)
    finally
        ccall((:lsm_iso_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), s)
    end
end

# mesh_distance!: ϕ := the signed distance to a closed, consistently oriented mesh, cut off at `cutoff` (include/lsm.h,
# lsm_mesh_distance) — the inverse of isosurface_arrays.  vertices ndim x nv Float64 and elements ndim x ne Int64 with 0-based
# vertex numbers, both on the device.  Returns (near, unbalanced, skipped); unbalanced != 0: the mesh is open or inconsistently
# oriented as seen from that many grid rows.
function mesh_distance!(ϕ::ROCMeshField, vertices::ROCMatrix{Float64}, elements::ROCMatrix{Int64}; cutoff = Inf)
    stats = zeros(Int64, 3)
    _check(ϕ.h.ptr, ccall((:lsm_mesh_distance, libhiplsm), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Float64, Ptr{Cvoid}, Ptr{Int64}, Ptr{Cvoid}),
        ϕ.h.ptr, size(vertices, 2), pointer(vertices), size(elements, 2), pointer(elements), cutoff, pointer(ϕ.buf), stats, C_NULL), "lsm_mesh_distance")
    stats[2] == 0 || error("mesh_distance: the mesh is not closed or not consistently oriented ($(stats[2]) grid rows see unbalanced crossings)")
    return (; near = stats[1], unbalanced = stats[2], skipped = stats[3])
end

# eikonal!: ϕ := copysign(min(T, cutoff), ϕ), T the first-order solution of |∇T| = 1/speed over the whole grid (include/lsm.h,
# lsm_eikonal): the far-field signed distance (speed = nothing) or travel times (speed: one Float64 per interior node on the
# device, n-shaped).  width = 0: the crossing seed; width = w > 0: the nodes with |ϕ| <= w keep |ϕ|.  Returns (frozen, iterations,
# visits, clamped).
function eikonal!(ϕ::ROCMeshField; speed = nothing, width = 0.0, cutoff = Inf, max_iters = 0)
    stats = zeros(Int64, 4)
    _check(ϕ.h.ptr, ccall((:lsm_eikonal, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Float64, Float64, Int64, Ptr{Int64}, Ptr{Cvoid}),
        ϕ.h.ptr, pointer(ϕ.buf), speed === nothing ? C_NULL : pointer(speed), width, cutoff, max_iters, stats, C_NULL), "lsm_eikonal")
    return (; frozen = stats[1], iterations = stats[2], visits = stats[3], clamped = stats[4])
end

# extend_from_interface!: the fields Fs (one ROCMeshField or a vector of 1…8, on ϕ's handle) carried off a frozen set along the
# characteristics of |ϕ| (include/lsm.h, lsm_extend), in place; ϕ is read only.  frozen = nothing: eikonal!'s seeding set for the
# same width; :inside (ϕ <= 0), :outside (ϕ >= 0), or a ROCVector{UInt8} with one byte per interior node (non-zero: frozen).
# source = :nodes or :interface (the values at the crossings; with frozen = nothing only).  Returns (frozen, iterations, visits,
# orphans, filled).
function extend_from_interface!(Fs, ϕ::ROCMeshField; width = 0.0, frozen = nothing, source = :nodes, cutoff = Inf, fill = 0.0, max_iters = 0)
    fields = Fs isa ROCMeshField ? [Fs] : collect(Fs)
    ptrs = Ptr{Cvoid}[pointer(F.buf) for F in fields]
    rule = frozen === nothing ? 0 : frozen === :inside ? 2 : frozen === :outside ? 3 : 1
    stats = zeros(Int64, 5)
    _check(ϕ.h.ptr, ccall((:lsm_extend, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Cint, Cint, Ptr{UInt8}, Float64, Cint, Float64, Float64, Int64, Ptr{Int64}, Ptr{Cvoid}),
        ϕ.h.ptr, pointer(ϕ.buf), ptrs, length(fields), rule, rule == 1 ? pointer(frozen) : C_NULL, width, source === :interface ? 1 : 0, cutoff, fill,
        max_iters, stats, C_NULL), "lsm_extend")
    return (; frozen = stats[1], iterations = stats[2], visits = stats[3], orphans = stats[4], filled = stats[5])
end

# components: the connected components of {ϕ < level} (side = :inside) or of its complement (:outside) over the Kuhn edges
# (include/lsm.h, lsm_cc_*), numbered by their smallest linear node index.  Returns the object `cc` (release it with
# destroy_components; remove_components! needs it), count, labels (Int32, one per node, −1 off the set, on the device), nodes
# (K), index_sums (ndim x K, of the 0-based indices) and bbox (ndim x 2 x K, 0-based), and the call's stats.
function components(ϕ::ROCMeshField; level = 0.0, side = :inside)
    out, stats = Ref{Ptr{Cvoid}}(), zeros(Int64, 4)
    _check(ϕ.h.ptr, ccall((:lsm_cc_create, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), level, side === :outside ? 1 : 0, out, stats), "lsm_cc_create")
    cc, K, N = out[], stats[1], ndims(ϕ)
    labels = ROCArray{Int32}(undef, size(ϕ.mesh)...)
    nodes, index_sums, bbox = ROCVector{Int64}(undef, K), ROCMatrix{Int64}(undef, N, K), ROCArray{Int32}(undef, N, 2, K)
    _check(ϕ.h.ptr, ccall((:lsm_cc_read, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        cc, pointer(labels), K == 0 ? C_NULL : pointer(nodes), K == 0 ? C_NULL : pointer(index_sums), K == 0 ? C_NULL : pointer(bbox)), "lsm_cc_read")
    return (; cc, count = K, labels, nodes, index_sums, bbox, stats)
end

# remove_components!: every node of the components flagged in `which` (K bytes on the device) is mirrored to the other side of
# the level, in place; refused with ϕ untouched when ϕ no longer matches `c`.  Not a distance function afterwards near what was
# removed: reinitialize! or eikonal! next.  Returns the number of nodes flipped.
function remove_components!(ϕ::ROCMeshField, c, which::ROCVector{UInt8})
    length(which) == c.count || throw(ArgumentError("which has $(length(which)) entries, there are $(c.count) components"))
    c.count == 0 && return 0
    flipped = Ref{Int64}(0)
    _check(ϕ.h.ptr, ccall((:lsm_cc_flip, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}),
        c.cc, pointer(ϕ.buf), pointer(which), flipped), "lsm_cc_flip")
    return flipped[]
end

destroy_components(c) = ccall((:lsm_cc_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), c.cc)

# elliptic_operator: the discrete −∇·(a∇u) + c·u of ϕ's grid with its multigrid hierarchy (include/lsm.h, lsm_elliptic_*).  The cell
# coefficient is a_out + (a_in − a_out)·θ(ϕ), or `a` (a ROCArray{Float64} of size n .- 1); c: a number or a ROCArray{Float64} of
# the grid's size; fixed: nothing or a ROCArray{UInt8} of the grid's size (non-zero = Dirichlet node); precond :mg or :jacobi.
# Release it with destroy_elliptic.
function elliptic_operator(ϕ::ROCMeshField; level = 0.0, a_in = 1.0, a_out = 1e-3, a = nothing, c = 0.0, fixed = nothing, precond = :mg)
    out, stats = Ref{Ptr{Cvoid}}(), zeros(Int64, 4)
    cnodes = c isa Number ? C_NULL : pointer(c)
    _check(ϕ.h.ptr, ccall((:lsm_elliptic_create, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), level, a_in, a_out, a === nothing ? C_NULL : pointer(a), c isa Number ? Float64(c) : 0.0, cnodes,
        fixed === nothing ? C_NULL : pointer(fixed), precond === :jacobi ? 1 : 0, out, stats), "lsm_elliptic_create")
    return (; op = out[], h = ϕ.h, levels = stats[1], free = stats[2], fixed = stats[3])
end

# elliptic_solve!: u (a field of the same handle) holds the guess and, on the fixed nodes, the Dirichlet values; on return the
# solution.  f: a ROCArray{Float64} of the grid's size.  Returns (iterations, relres); a failure leaves u untouched.
function elliptic_solve!(u::ROCMeshField, E, f; rtol = 1e-8, max_iters = 500)
    iters, relres = Ref{Cint}(0), Ref{Float64}(0.0)
    _check(E.h.ptr, ccall((:lsm_elliptic_solve, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Float64, Cint, Ref{Cint}, Ref{Float64}, Ptr{Cvoid}),
        E.op, pointer(f), pointer(u.buf), rtol, max_iters, iters, relres, C_NULL), "lsm_elliptic_solve")
    return (; iterations = iters[], relres = relres[])
end

# y = A x on all nodes, no elimination (x, y: ROCArray{Float64} of the grid's size)
elliptic_apply!(y, E, x) = _check(E.h.ptr, ccall((:lsm_elliptic_apply, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), E.op, pointer(x), pointer(y)), "lsm_elliptic_apply")

# the energy density a|∇u|² at the nodes into the field e: the normal speed of a compliance descent (NormalMotionTerm takes e.buf's values)
elliptic_energy!(e::ROCMeshField, E, u::ROCMeshField) =
    _check(E.h.ptr, ccall((:lsm_elliptic_energy, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), E.op, pointer(u.buf), pointer(e.buf)), "lsm_elliptic_energy")

function elliptic_compliance(E, f, u::ROCMeshField)
    out = Ref{Float64}(0.0)
    _check(E.h.ptr, ccall((:lsm_elliptic_compliance, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Ref{Float64}), E.op, pointer(f), pointer(u.buf), out), "lsm_elliptic_compliance")
    return out[]
end

# the level-0 cell coefficients into a ROCArray{Float64} of size n .- 1
elliptic_cells!(a, E) = _check(E.h.ptr, ccall((:lsm_elliptic_cells, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), E.op, pointer(a)), "lsm_elliptic_cells")

# elliptic_solve_many!: K ≤ 8 sources of one operator in one batched solve.  us: K fields (guess and Dirichlet values in, solutions out);
# f: a ROCArray{Float64} of K·nn values, column k at (k-1)·nn.  Column k is elliptic_solve! of column k bit for bit.  Returns the K
# iteration counts, residuals and statuses; unless every column converges it throws and leaves every field untouched.
function elliptic_solve_many!(us, E, f; rtol = 1e-8, max_iters = 500)
    nk = length(us)
    iters, relres, status = zeros(Cint, nk), zeros(Float64, nk), zeros(Cint, nk)
    p = Ptr{Cvoid}[pointer(u.buf) for u in us]
    _check(E.h.ptr, ccall((:lsm_elliptic_solve_many, libhiplsm), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Ptr{Cvoid}}, Float64, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Cint}, Ptr{Cvoid}),
        E.op, nk, pointer(f), p, rtol, max_iters, iters, relres, status, C_NULL), "lsm_elliptic_solve_many")
    return (; iterations = iters, relres = relres, status = status)
end

# Σ_k w_k·(the energy density of column k) into the field e, in one pass: the normal speed of a weighted multi-source compliance descent
function elliptic_energy_many!(e::ROCMeshField, E, us, w)
    p, wv = Ptr{Cvoid}[pointer(u.buf) for u in us], collect(Float64, w)
    _check(E.h.ptr, ccall((:lsm_elliptic_energy_many, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Cvoid}),
        E.op, length(us), p, wv, pointer(e.buf)), "lsm_elliptic_energy_many")
end

# the mutual energy density a∇u·∇v at the nodes into the field e (without the c·u·v term): the shape-derivative integrand of l·u for the adjoint A v = l
elliptic_energy_mutual!(e::ROCMeshField, E, u::ROCMeshField, v::ROCMeshField) =
    _check(E.h.ptr, ccall((:lsm_elliptic_energy_mutual, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        E.op, pointer(u.buf), pointer(v.buf), pointer(e.buf)), "lsm_elliptic_energy_mutual")

destroy_elliptic(E) = ccall((:lsm_elliptic_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), E.op)

# elasticity_operator: the discrete Q1 operator of −∇·σ(u), σ = E(x)·C₀(ν):ε(u), on ϕ's grid with its multigrid hierarchy
# (include/lsm.h, lsm_elastic_*).  The cell modulus is E_out + (E_in − E_out)·θ(ϕ), or `E` (a ROCArray{Float64} of size n .- 1);
# plane :stress or :strain (2-D only); fixed: a ROCArray{UInt8} of the grid's size, bit i-1 set = component i keeps its value (every
# component needs one somewhere); precond :mg or :jacobi.  Release it with destroy_elasticity.
function elasticity_operator(ϕ::ROCMeshField, fixed; level = 0.0, E_in = 1.0, E_out = 1e-3, E = nothing, nu = 0.3, plane = :stress, precond = :mg)
    out, stats = Ref{Ptr{Cvoid}}(), zeros(Int64, 4)
    _check(ϕ.h.ptr, ccall((:lsm_elastic_create, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Float64}, Float64, Cint, Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), level, E_in, E_out, E === nothing ? C_NULL : pointer(E), nu, plane === :strain ? 1 : 0,
        pointer(fixed), precond === :jacobi ? 1 : 0, out, stats), "lsm_elastic_create")
    return (; op = out[], h = ϕ.h, levels = stats[1], free = stats[2], fixed = stats[3])
end

_u3(u) = (pointer(u[1].buf), pointer(u[2].buf), length(u) > 2 ? pointer(u[3].buf) : C_NULL)

# elasticity_solve!: u, a tuple of N fields of the same handle, holds the guess and, on the fixed components, the prescribed values;
# on return the solution.  f: a ROCArray{Float64} of N·nn values, component-major.  Returns (iterations, relres); a failure leaves u
# untouched.
function elasticity_solve!(u, K, f; rtol = 1e-8, max_iters = 500)
    iters, relres = Ref{Cint}(0), Ref{Float64}(0.0)
    p = _u3(u)
    _check(K.h.ptr, ccall((:lsm_elastic_solve, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Cint, Ref{Cint}, Ref{Float64}, Ptr{Cvoid}),
        K.op, pointer(f), p[1], p[2], p[3], rtol, max_iters, iters, relres, C_NULL), "lsm_elastic_solve")
    return (; iterations = iters[], relres = relres[])
end

# y = A x on all components, no elimination (x, y: ROCArray{Float64} of N·nn values, component-major)
elasticity_apply!(y, K, x) = _check(K.h.ptr, ccall((:lsm_elastic_apply, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), K.op, pointer(x), pointer(y)), "lsm_elastic_apply")

# the unit element matrix of a level as the device holds it: a (2^N·N)² host matrix (row-major in C: the matrix is symmetric)
function elasticity_stiffness(K, level, N)
    R = (1 << N) * N
    k0 = zeros(Float64, R, R)
    _check(K.h.ptr, ccall((:lsm_elastic_stiffness, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), K.op, level, k0), "lsm_elastic_stiffness")
    return k0
end

# the energy density E·C₀ε:ε at the nodes into the field e: the normal speed of a compliance descent
function elasticity_energy!(e::ROCMeshField, K, u)
    p = _u3(u)
    _check(K.h.ptr, ccall((:lsm_elastic_energy, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), K.op, p[1], p[2], p[3], pointer(e.buf)), "lsm_elastic_energy")
end

function elasticity_compliance(K, f, u)
    out = Ref{Float64}(0.0)
    p = _u3(u)
    _check(K.h.ptr, ccall((:lsm_elastic_compliance, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Float64}), K.op, pointer(f), p[1], p[2], p[3], out), "lsm_elastic_compliance")
    return out[]
end

# the level-0 cell moduli into a ROCArray{Float64} of size n .- 1
elasticity_cells!(a, K) = _check(K.h.ptr, ccall((:lsm_elastic_cells, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), K.op, pointer(a)), "lsm_elastic_cells")

# the field pointers of K columns of N fields each, column by column (include/lsm.h: u[k·N + i])
_ucols(us) = Ptr{Cvoid}[pointer(c.buf) for u in us for c in u]

# elasticity_solve_many!: K ≤ 8 load cases of one operator in one batched solve.  us: K tuples of N fields (guess and prescribed values in,
# solutions out); f: a ROCArray{Float64} of K·N·nn values, column k at (k-1)·N·nn.  Column k is elasticity_solve! of column k bit for bit.
# Returns the K iteration counts, residuals and statuses; unless every column converges it throws and leaves every field untouched.
function elasticity_solve_many!(us, K, f; rtol = 1e-8, max_iters = 500)
    nk = length(us)
    iters, relres, status = zeros(Cint, nk), zeros(Float64, nk), zeros(Cint, nk)
    p = _ucols(us)
    _check(K.h.ptr, ccall((:lsm_elastic_solve_many, libhiplsm), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Ptr{Cvoid}}, Float64, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Cint}, Ptr{Cvoid}),
        K.op, nk, pointer(f), p, rtol, max_iters, iters, relres, status, C_NULL), "lsm_elastic_solve_many")
    return (; iterations = iters, relres = relres, status = status)
end

# Σ_k w_k·(the energy density of column k) into the field e, in one pass: the normal speed of a weighted multi-load compliance descent
function elasticity_energy_many!(e::ROCMeshField, K, us, w)
    p, wv = _ucols(us), collect(Float64, w)
    _check(K.h.ptr, ccall((:lsm_elastic_energy_many, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Cvoid}),
        K.op, length(us), p, wv, pointer(e.buf)), "lsm_elastic_energy_many")
end

# the mutual energy density E·C₀ε(u):ε(v) at the nodes into the field e: the shape-derivative integrand of l·u for the adjoint K v = l
function elasticity_energy_mutual!(e::ROCMeshField, K, u, v)
    p, q = _u3(u), _u3(v)
    _check(K.h.ptr, ccall((:lsm_elastic_energy_mutual, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        K.op, p[1], p[2], p[3], q[1], q[2], q[3], pointer(e.buf)), "lsm_elastic_energy_mutual")
end

destroy_elasticity(K) = ccall((:lsm_elastic_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), K.op)

# homogenize: the effective elasticity tensor of the periodic material whose cell is the box of ϕ (include/lsm.h, lsm_homog_*).  The torus
# has m = n .- 1 nodes per axis; M = N(N+1)/2 unit strains in Voigt order.  Release the object with destroy_homogenization.
function homogenization(ϕ::ROCMeshField; level = 0.0, E_in = 1.0, E_out = 1e-3, E = nothing, nu = 0.3, plane = :stress, precond = :mg)
    out, stats = Ref{Ptr{Cvoid}}(), zeros(Int64, 4)
    _check(ϕ.h.ptr, ccall((:lsm_homog_create, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Float64}, Float64, Cint, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), level, E_in, E_out, E === nothing ? C_NULL : pointer(E), nu, plane === :strain ? 1 : 0,
        precond === :jacobi ? 1 : 0, out, stats), "lsm_homog_create")
    return (; op = out[], h = ϕ.h, levels = stats[1], free = stats[2], nodes = stats[3])
end

function homogenization_stiffness(H, level, N)
    R = (1 << N) * N
    k0 = zeros(Float64, R, R)
    _check(H.h.ptr, ccall((:lsm_homog_stiffness, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), H.op, level, k0), "lsm_homog_stiffness")
    return k0
end

# the cell moduli into a ROCArray{Float64} of size n .- 1; y = A x and the load of unit strain k (0-based) over ROCArray{Float64}s of N·nn values
homogenization_cells!(a, H) = _check(H.h.ptr, ccall((:lsm_homog_cells, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), H.op, pointer(a)), "lsm_homog_cells")
homogenization_apply!(y, H, x) = _check(H.h.ptr, ccall((:lsm_homog_apply, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), H.op, pointer(x), pointer(y)), "lsm_homog_apply")
homogenization_load!(f, H, k) = _check(H.h.ptr, ccall((:lsm_homog_load, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), H.op, k, pointer(f)), "lsm_homog_load")

# all M correctors, from `guess` (a Float64 array of M·N·nn values, host or device) or from zero; a failure leaves the stored ones untouched
function homogenization_solve!(H, M; guess = nothing, rtol = 1e-8, max_iters = 500)
    iters, relres = zeros(Cint, M), zeros(Float64, M)
    _check(H.h.ptr, ccall((:lsm_homog_solve, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64, Cint, Ptr{Cint}, Ptr{Float64}),
        H.op, guess === nothing ? C_NULL : pointer(guess), rtol, max_iters, iters, relres), "lsm_homog_solve")
    return (; iterations = iters, relres = relres)
end

# A x = f away from the pinned node for a right-hand side of the caller's (x, f: ROCArray{Float64} of N·nn values; x holds the guess, then the solution)
function homogenization_solve_rhs!(x, H, f; rtol = 1e-8, max_iters = 500)
    iters, relres = Ref{Cint}(0), Ref{Float64}(0.0)
    _check(H.h.ptr, ccall((:lsm_homog_solve_rhs, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Cint, Ref{Cint}, Ref{Float64}),
        H.op, pointer(f), pointer(x), rtol, max_iters, iters, relres), "lsm_homog_solve_rhs")
    return (; iterations = iters[], relres = relres[])
end

homogenization_set_correctors!(H, chi) = _check(H.h.ptr, ccall((:lsm_homog_set_correctors, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), H.op, pointer(chi)), "lsm_homog_set_correctors")
homogenization_correctors!(chi, H) = _check(H.h.ptr, ccall((:lsm_homog_correctors, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), H.op, pointer(chi)), "lsm_homog_correctors")
homogenization_energy_cells!(t, H, p, q) = _check(H.h.ptr, ccall((:lsm_homog_energy_cells, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}), H.op, p, q, pointer(t)), "lsm_homog_energy_cells")

# C^H, an M×M host matrix (symmetric)
function homogenization_tensor(H, M)
    C = zeros(Float64, M, M)
    _check(H.h.ptr, ccall((:lsm_homog_tensor, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), H.op, C), "lsm_homog_tensor")
    return C
end

# corrector k (0-based) into the N fields u; the integrand of d(W:C^H)/dΩ into the field g: the normal speed of a descent on W:C^H
function homogenization_corrector!(u, H, k)
    p = _u3(u)
    _check(H.h.ptr, ccall((:lsm_homog_corrector, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), H.op, k, p[1], p[2], p[3]), "lsm_homog_corrector")
end
homogenization_sensitivity!(g::ROCMeshField, H, W::Matrix{Float64}) = _check(H.h.ptr, ccall((:lsm_homog_sensitivity, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}), H.op, W, pointer(g.buf)), "lsm_homog_sensitivity")

destroy_homogenization(H) = ccall((:lsm_homog_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), H.op)

# homogenize_conductivity: the effective conductivity tensor of −∇·(a∇u) for the periodic material whose cell is the box of ϕ (include/lsm.h,
# lsm_hcond_*).  The torus has m = n .- 1 nodes per axis; N unit gradients.  Release the object with destroy_conductivity_homogenization.
function conductivity_homogenization(ϕ::ROCMeshField; level = 0.0, a_in = 1.0, a_out = 1e-3, a = nothing, precond = :mg)
    out, stats = Ref{Ptr{Cvoid}}(), zeros(Int64, 4)
    _check(ϕ.h.ptr, ccall((:lsm_hcond_create, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}, Ptr{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), level, a_in, a_out, a === nothing ? C_NULL : pointer(a), precond === :jacobi ? 1 : 0, out, stats), "lsm_hcond_create")
    return (; op = out[], h = ϕ.h, levels = stats[1], free = stats[2], nodes = stats[3])
end

# the cell coefficients into a ROCArray{Float64} of size n .- 1; y = A x and the load of unit gradient k (0-based) over ROCArray{Float64}s of nn values
conductivity_homogenization_cells!(a, H) = _check(H.h.ptr, ccall((:lsm_hcond_cells, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), H.op, pointer(a)), "lsm_hcond_cells")
conductivity_homogenization_apply!(y, H, x) = _check(H.h.ptr, ccall((:lsm_hcond_apply, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), H.op, pointer(x), pointer(y)), "lsm_hcond_apply")
conductivity_homogenization_load!(f, H, k) = _check(H.h.ptr, ccall((:lsm_hcond_load, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), H.op, k, pointer(f)), "lsm_hcond_load")

# all N correctors, from `guess` (a Float64 array of N·nn values, host or device) or from zero; a failure leaves the stored ones untouched
function conductivity_homogenization_solve!(H, N; guess = nothing, rtol = 1e-8, max_iters = 500)
    iters, relres = zeros(Cint, N), zeros(Float64, N)
    _check(H.h.ptr, ccall((:lsm_hcond_solve, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64, Cint, Ptr{Cint}, Ptr{Float64}),
        H.op, guess === nothing ? C_NULL : pointer(guess), rtol, max_iters, iters, relres), "lsm_hcond_solve")
    return (; iterations = iters, relres = relres)
end

# A x = f away from the pinned node for a right-hand side of the caller's (x, f: ROCArray{Float64} of nn values; x holds the guess, then the solution)
function conductivity_homogenization_solve_rhs!(x, H, f; rtol = 1e-8, max_iters = 500)
    iters, relres = Ref{Cint}(0), Ref{Float64}(0.0)
    _check(H.h.ptr, ccall((:lsm_hcond_solve_rhs, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Cint, Ref{Cint}, Ref{Float64}),
        H.op, pointer(f), pointer(x), rtol, max_iters, iters, relres), "lsm_hcond_solve_rhs")
    return (; iterations = iters[], relres = relres[])
end

conductivity_homogenization_set_correctors!(H, chi) = _check(H.h.ptr, ccall((:lsm_hcond_set_correctors, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), H.op, pointer(chi)), "lsm_hcond_set_correctors")
conductivity_homogenization_correctors!(chi, H) = _check(H.h.ptr, ccall((:lsm_hcond_correctors, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), H.op, pointer(chi)), "lsm_hcond_correctors")
conductivity_homogenization_energy_cells!(t, H, p, q) = _check(H.h.ptr, ccall((:lsm_hcond_energy_cells, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}), H.op, p, q, pointer(t)), "lsm_hcond_energy_cells")

# K^H, an N×N host matrix (symmetric)
function conductivity_homogenization_tensor(H, N)
    K = zeros(Float64, N, N)
    _check(H.h.ptr, ccall((:lsm_hcond_tensor, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), H.op, K), "lsm_hcond_tensor")
    return K
end

# corrector k (0-based) into the field u; the integrand of d(W:K^H)/dΩ into the field g: the normal speed of a descent on W:K^H
conductivity_homogenization_corrector!(u::ROCMeshField, H, k) = _check(H.h.ptr, ccall((:lsm_hcond_corrector, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), H.op, k, pointer(u.buf)), "lsm_hcond_corrector")
conductivity_homogenization_sensitivity!(g::ROCMeshField, H, W::Matrix{Float64}) = _check(H.h.ptr, ccall((:lsm_hcond_sensitivity, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}), H.op, W, pointer(g.buf)), "lsm_hcond_sensitivity")

destroy_conductivity_homogenization(H) = ccall((:lsm_hcond_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), H.op)

# elasticity_modes: the m ≤ 8 lowest vibration modes K u = λ M u of an elasticity_operator K (include/lsm.h, lsm_elastic_modes_*).  The
# density of a cell is rho_out + (rho_in − rho_out)·θ(ϕ), or `rho` (a ROCArray{Float64} of size n .- 1, required when K was built from
# `E`).  The object borrows K, which must outlive it; release it with destroy_modes.
function elasticity_modes(K, ϕ::ROCMeshField, m; level = 0.0, rho_in = 1.0, rho_out = 1e-6, rho = nothing)
    out = Ref{Ptr{Cvoid}}()
    _check(K.h.ptr, ccall((:lsm_elastic_modes_create, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
        K.op, rho === nothing ? pointer(ϕ.buf) : C_NULL, level, rho_in, rho_out, rho === nothing ? C_NULL : pointer(rho), m, out), "lsm_elastic_modes_create")
    return (; md = out[], h = K.h, m = m)
end

# modes_solve!: LOBPCG from x0 (a ROCArray{Float64} of m·N·nn values, or nothing: the fixed pseudo-random start) until every mode's
# relative residual is below rtol.  Returns (eigenvalues, relres, iterations); LSM_ERR_NOT_CONVERGED throws, the last iterate stays.
function modes_solve!(M; x0 = nothing, rtol = 1e-6, max_iters = 300)
    lam, rel, iters, stats = zeros(Float64, M.m), zeros(Float64, M.m), Ref{Cint}(0), zeros(Int64, 4)
    _check(M.h.ptr, ccall((:lsm_elastic_modes_solve, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64, Cint, Ptr{Float64}, Ptr{Float64}, Ref{Cint}, Ptr{Int64}),
        M.md, x0 === nothing ? C_NULL : pointer(x0), rtol, max_iters, lam, rel, iters, stats), "lsm_elastic_modes_solve")
    return (; eigenvalues = lam, relres = rel, iterations = iters[])
end

# the node mass into a ROCArray{Float64} of the grid's size; X into one of m·N·nn values (the next design's x0)
modes_mass!(a, M) = _check(M.h.ptr, ccall((:lsm_elastic_modes_mass, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), M.md, pointer(a)), "lsm_elastic_modes_mass")
modes_vectors!(x, M) = _check(M.h.ptr, ccall((:lsm_elastic_modes_vectors, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), M.md, pointer(x)), "lsm_elastic_modes_vectors")

# mode k (0-based, as in C) into the N fields u, normalised to ∫ρ|u|² = 1; its shape-derivative integrand into the field g
function modes_store!(u, M, k)
    p = _u3(u)
    _check(M.h.ptr, ccall((:lsm_elastic_modes_store, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), M.md, k, p[1], p[2], p[3]), "lsm_elastic_modes_store")
end
modes_sensitivity!(g::ROCMeshField, M, k) =
    _check(M.h.ptr, ccall((:lsm_elastic_modes_sensitivity, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), M.md, k, pointer(g.buf)), "lsm_elastic_modes_sensitivity")

destroy_modes(M) = ccall((:lsm_elastic_modes_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), M.md)

# elliptic_modes: the m ≤ 8 lowest eigenmodes A u = λ M u of an elliptic_operator A, its c term included (include/lsm.h,
# lsm_elliptic_modes_*): cavity resonances, membrane tones, the principal eigenvalue.  The density of a cell is
# rho_out + (rho_in − rho_out)·θ(ϕ), or `rho` (a ROCArray{Float64} of size n .- 1, required when A was built from `a`).  The object
# borrows A, which must outlive it; release it with destroy_elliptic_modes.
function elliptic_modes(A, ϕ::ROCMeshField, m; level = 0.0, rho_in = 1.0, rho_out = 1e-6, rho = nothing)
    out = Ref{Ptr{Cvoid}}()
    _check(A.h.ptr, ccall((:lsm_elliptic_modes_create, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Float64}, Cint, Ref{Ptr{Cvoid}}),
        A.op, rho === nothing ? pointer(ϕ.buf) : C_NULL, level, rho_in, rho_out, rho === nothing ? C_NULL : pointer(rho), m, out), "lsm_elliptic_modes_create")
    return (; md = out[], h = A.h, m = m)
end

# elliptic_modes_solve!: LOBPCG from x0 (a ROCArray{Float64} of m·nn values, or nothing: the fixed pseudo-random start) until every
# mode's relative residual is below rtol.  Returns (eigenvalues, relres, iterations); LSM_ERR_NOT_CONVERGED throws, the last iterate stays.
function elliptic_modes_solve!(M; x0 = nothing, rtol = 1e-6, max_iters = 300)
    lam, rel, iters, stats = zeros(Float64, M.m), zeros(Float64, M.m), Ref{Cint}(0), zeros(Int64, 4)
    _check(M.h.ptr, ccall((:lsm_elliptic_modes_solve, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64, Cint, Ptr{Float64}, Ptr{Float64}, Ref{Cint}, Ptr{Int64}),
        M.md, x0 === nothing ? C_NULL : pointer(x0), rtol, max_iters, lam, rel, iters, stats), "lsm_elliptic_modes_solve")
    return (; eigenvalues = lam, relres = rel, iterations = iters[])
end

# the node mass into a ROCArray{Float64} of the grid's size; X into one of m·nn values (the next design's x0); y = A x for ncols ≤ 8
# columns of nn values, x zero on the fixed nodes (the solve's block apply)
elliptic_modes_mass!(a, M) = _check(M.h.ptr, ccall((:lsm_elliptic_modes_mass, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), M.md, pointer(a)), "lsm_elliptic_modes_mass")
elliptic_modes_vectors!(x, M) = _check(M.h.ptr, ccall((:lsm_elliptic_modes_vectors, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Float64}), M.md, pointer(x)), "lsm_elliptic_modes_vectors")
elliptic_modes_apply!(y, M, x, ncols) =
    _check(M.h.ptr, ccall((:lsm_elliptic_modes_apply, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}), M.md, ncols, pointer(x), pointer(y)), "lsm_elliptic_modes_apply")

# mode k (0-based, as in C) into the field u, normalised to ∫ρu² = 1; its shape-derivative integrand into the field g
elliptic_modes_store!(u::ROCMeshField, M, k) =
    _check(M.h.ptr, ccall((:lsm_elliptic_modes_store, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), M.md, k, pointer(u.buf)), "lsm_elliptic_modes_store")
elliptic_modes_sensitivity!(g::ROCMeshField, M, k) =
    _check(M.h.ptr, ccall((:lsm_elliptic_modes_sensitivity, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), M.md, k, pointer(g.buf)), "lsm_elliptic_modes_sensitivity")

destroy_elliptic_modes(M) = ccall((:lsm_elliptic_modes_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), M.md)

# Stress recovery of a displacement u (N fields; any displacement, not only a solution) on an elasticity_operator K (include/lsm.h,
# lsm_elastic_stress_*).  `what`: 0 the strain, 1 the stress (both N(N+1)/2 components in Voigt order: 2-D (00, 11, 01), 3-D (00, 11,
# 22, 12, 02, 01)), 2 the von Mises stress (one component).
const LSM_STRESS_STRAIN, LSM_STRESS_STRESS, LSM_STRESS_VON_MISES = 0, 1, 2

# the cell arrays, component-major, into a ROCArray{Float64} of M·prod(n .- 1) values (or prod(n .- 1) for the von Mises stress)
function stress_cells!(a, K, u, what)
    p = _u3(u)
    _check(K.h.ptr, ccall((:lsm_elastic_stress_cells, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}),
        K.op, p[1], p[2], p[3], what, pointer(a)), "lsm_elastic_stress_cells")
end

# the node fields (the mean over the cells around a node) into the tuple `out` of M distinct fields (one for the von Mises stress)
function stress_fields!(out, K, u, what)
    p = _u3(u)
    o = ntuple(k -> k <= length(out) ? pointer(out[k].buf) : C_NULL, 6)
    _check(K.h.ptr, ccall((:lsm_elastic_stress, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        K.op, p[1], p[2], p[3], what, o[1], o[2], o[3], o[4], o[5], o[6]), "lsm_elastic_stress")
end

# (J′, smax): J′ = Σ_C (s_C/sref)^p for 2 ≤ p ≤ 64, reduced on the device, and the largest cell stress.  The p-norm is
# G_p = sref·(prod(h)·J′)^(1/p).
function stress_norm(K, u, p, sref)
    out = zeros(Float64, 2)
    q = _u3(u)
    _check(K.h.ptr, ccall((:lsm_elastic_stress_norm, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}),
        K.op, q[1], q[2], q[3], p, sref, out), "lsm_elastic_stress_norm")
    return (; J = out[1], smax = out[2])
end

# the adjoint load ∂J′/∂u as elasticity_solve!'s f (a ROCArray{Float64} of N·nn values): solve with zero values on the fixed components
function stress_load!(f, K, u, p, sref)
    q = _u3(u)
    _check(K.h.ptr, ccall((:lsm_elastic_stress_load, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}),
        K.op, q[1], q[2], q[3], p, sref, pointer(f)), "lsm_elastic_stress_load")
end

# the sensitivity into the field g from the state u and the adjoint λ (N fields each): with scale = G_p/(p·J′) it is E_C·∂G_p/∂E_C
# averaged over the cells around a node, the convention of elasticity_energy!
function stress_sensitivity!(g::ROCMeshField, K, u, λ, p, sref, scale)
    q, l = _u3(u), _u3(λ)
    _check(K.h.ptr, ccall((:lsm_elastic_stress_sensitivity, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Ptr{Cvoid}),
        K.op, q[1], q[2], q[3], l[1], l[2], l[3], p, sref, scale, pointer(g.buf)), "lsm_elastic_stress_sensitivity")
end

# Topological derivative of the compliance for a displacement u on an elasticity_operator K (include/lsm.h, lsm_elastic_topo*): the
# cost per unit volume of a small traction-free hole.  The cell array into a ROCArray{Float64} of prod(n .- 1) values; the node field
# (the mean over the cells around a node) into the field g, distinct from the fields of u.
function topological_derivative_cells!(a, K, u)
    p = _u3(u)
    _check(K.h.ptr, ccall((:lsm_elastic_topo_cells, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}),
        K.op, p[1], p[2], p[3], pointer(a)), "lsm_elastic_topo_cells")
end
function topological_derivative!(g::ROCMeshField, K, u)
    p = _u3(u)
    _check(K.h.ptr, ccall((:lsm_elastic_topo, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        K.op, p[1], p[2], p[3], pointer(g.buf)), "lsm_elastic_topo")
    return g
end

# Thermoelastic coupling on an elasticity_operator K (include/lsm.h, lsm_elastic_thermal_*): T a temperature field, t_ref the stress-free
# temperature, alpha the expansion coefficient — a number, or a ROCArray{Float64} of prod(n .- 1) cell values.
_alpha(alpha::Real) = (Float64(alpha), Ptr{Float64}(C_NULL))
_alpha(alpha) = (0.0, pointer(alpha))

# the load of the eigenstress E·C₀:(α(T − t_ref)I) as elasticity_solve!'s f (a ROCArray{Float64} of N·nn values)
function thermal_load!(f, K, T::ROCMeshField, t_ref, alpha)
    a = _alpha(alpha)
    _check(K.h.ptr, ccall((:lsm_elastic_thermal_load, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}, Ptr{Float64}),
        K.op, pointer(T.buf), t_ref, a[1], a[2], pointer(f)), "lsm_elastic_thermal_load")
end

# the stress recovery with the thermal strain taken off (`what`: LSM_STRESS_STRESS or LSM_STRESS_VON_MISES): the cell arrays, and the
# node fields into the tuple `out`.  The von Mises stress differs from the isothermal one in plane stress only.
function thermal_stress_cells!(a, K, u, T::ROCMeshField, t_ref, alpha, what)
    p, al = _u3(u), _alpha(alpha)
    _check(K.h.ptr, ccall((:lsm_elastic_thermal_stress_cells, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}, Cint, Ptr{Float64}),
        K.op, p[1], p[2], p[3], pointer(T.buf), t_ref, al[1], al[2], what, pointer(a)), "lsm_elastic_thermal_stress_cells")
end
function thermal_stress_fields!(out, K, u, T::ROCMeshField, t_ref, alpha, what)
    p, al = _u3(u), _alpha(alpha)
    o = ntuple(k -> k <= length(out) ? pointer(out[k].buf) : C_NULL, 6)
    _check(K.h.ptr, ccall((:lsm_elastic_thermal_stress, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
        K.op, p[1], p[2], p[3], pointer(T.buf), t_ref, al[1], al[2], what, o[1], o[2], o[3], o[4], o[5], o[6]), "lsm_elastic_thermal_stress")
end

# the source of the heat adjoint from the elastic adjoint v (N fields), as elliptic_solve!'s f (a ROCArray{Float64} of nn values)
function thermal_source!(q, K, v, alpha)
    p, al = _u3(v), _alpha(alpha)
    _check(K.h.ptr, ccall((:lsm_elastic_thermal_source, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Float64}, Ptr{Float64}),
        K.op, p[1], p[2], p[3], al[1], al[2], pointer(q)), "lsm_elastic_thermal_source")
end

# the sensitivity of l·u into the field g from the state u, the elastic adjoint v and T; `minus` (a field, or nothing) is subtracted:
# the mutual energy density of the heat state and its adjoint when the temperature depends on the design
function thermal_sensitivity!(g::ROCMeshField, K, u, v, T::ROCMeshField, t_ref, alpha; minus = nothing)
    p, q, al = _u3(u), _u3(v), _alpha(alpha)
    m = minus === nothing ? C_NULL : pointer(minus.buf)
    _check(K.h.ptr, ccall((:lsm_elastic_thermal_sensitivity, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}),
        K.op, p[1], p[2], p[3], q[1], q[2], q[3], pointer(T.buf), t_ref, al[1], al[2], m, pointer(g.buf)), "lsm_elastic_thermal_sensitivity")
    return g
end

# Nucleation (include/lsm.h, lsm_nucleate_*).  find_nucleation_sites: the nodes where t < threshold and ϕ ≤ level − clearance whose
# (value, linear index) is the smallest among such nodes within ceil(spacing/h) nodes along every axis; returns the 0-based linear
# indices (ascending, on the device) and t at them.  punch!: a ball of `radius` removed around each of the 0-based linear node
# indices `centres` (a ROCVector{Int64}: those above, a part of them, the caller's own): ϕ ← max(ϕ, level + radius − |x − c|) over
# the ball's bounding box; returns the number of nodes changed.  Not a distance function afterwards: reinitialize! next.
# nucleate!: both, with the `max_holes` lowest centres by (value, index), spacing = 2·radius and clearance = radius by default.
function find_nucleation_sites(ϕ::ROCMeshField, t::ROCMeshField; threshold, radius, spacing = 2radius, clearance = radius, level = 0.0)
    out, count = Ref{Ptr{Cvoid}}(), Ref{Int64}(0)
    _check(ϕ.h.ptr, ccall((:lsm_nucleate_create, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Float64, Float64, Ref{Ptr{Cvoid}}, Ref{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), pointer(t.buf), threshold, level, clearance, spacing, out, count), "lsm_nucleate_create")
    K = count[]
    indices, values = ROCVector{Int64}(undef, K), ROCVector{Float64}(undef, K)
    code = K == 0 ? Cint(0) : ccall((:lsm_nucleate_read, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), out[], pointer(indices), pointer(values))
    ccall((:lsm_nucleate_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), out[])
    _check(ϕ.h.ptr, code, "lsm_nucleate_read")
    return (; indices, values)
end

function punch!(ϕ::ROCMeshField, centres::ROCVector{Int64}; radius, level = 0.0)
    changed = Ref{Int64}(0)
    _check(ϕ.h.ptr, ccall((:lsm_nucleate_punch, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Float64, Ref{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), isempty(centres) ? C_NULL : pointer(centres), length(centres), level, radius, changed), "lsm_nucleate_punch")
    return changed[]
end

function nucleate!(ϕ::ROCMeshField, t::ROCMeshField; threshold, radius, spacing = 2radius, clearance = radius, max_holes = nothing, level = 0.0)
    s = find_nucleation_sites(ϕ, t; threshold, radius, spacing, clearance, level)
    idx, val = Array(s.indices), Array(s.values)
    order = sortperm(collect(zip(val .+ 0.0, idx)))      # −0 and +0 are one value, as on the device
    max_holes === nothing || (order = order[1:min(max_holes, length(order))])
    centres = idx[order]
    changed = punch!(ϕ, ROCVector{Int64}(centres); radius, level)
    return (; centres, values = val[order], found = length(idx), changed)
end

# render: one picture of the interface {ϕ = level} (include/lsm.h, lsm_render_*; what ext/MakieExt.jl:142-171 draws), on the device.
# 3-D: `camera` = 13 Float64 (eye, forward, right·s_x, up·s_y, orthographic flag), `style` = 9 Float64 (colour, background, ambient,
# step, bisections); returns rgba 4 x W x H UInt8 (row 1 the top of the picture), depth W x H and normal 3 x W x H.  2-D: `camera`
# = nothing, `style` = 23 Float64 (line width, extent, the six class colours); returns rgba and cls W x H UInt8.  `mask`: a band
# field's byte mask.
function render_arrays(ϕ::ROCMeshField, camera; size = (640, 480), level = 0.0, mask = nothing,
        style = ndims(ϕ) == 3 ? Float64[70, 130, 180, 255, 255, 255, 0.25, 0.5, 6] :
                Float64[2, ϕ.mesh.lc[1], ϕ.mesh.hc[1], ϕ.mesh.lc[2], ϕ.mesh.hc[2], 255, 255, 255, 233, 233, 233, 0, 0, 0, 255, 255, 255, 198, 217, 234, 181, 198, 214])
    out = Ref{Ptr{Cvoid}}()
    _check(ϕ.h.ptr, ccall((:lsm_render_create, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ref{Ptr{Cvoid}}),
        ϕ.h.ptr, pointer(ϕ.buf), mask === nothing ? C_NULL : pointer(mask), level, out), "lsm_render_create")
    r = out[]
    try
        W, H = size
        rgba = ROCArray{UInt8}(undef, 4, W, H)
        three = ndims(ϕ) == 3
        aux = three ? ROCMatrix{Float64}(undef, W, H) : ROCMatrix{UInt8}(undef, W, H)
        normal = three ? ROCArray{Float64}(undef, 3, W, H) : nothing
        cam = camera === nothing ? nothing : convert(Vector{Float64}, camera)
        GC.@preserve cam _check(ϕ.h.ptr, ccall((:lsm_render_draw, libhiplsm), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Cint, Cint, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            r, cam === nothing ? Ptr{Float64}(C_NULL) : pointer(cam), W, H, style, pointer(rgba), pointer(aux), normal === nothing ? C_NULL : pointer(normal), C_NULL), "lsm_render_draw")
        _check(ϕ.h.ptr, ccall((:lsm_sync, libhiplsm), Cint, (Ptr{Cvoid},), ϕ.h.ptr), "lsm_sync")
        return three ? (; rgba, depth = aux, normal) : (; rgba, cls = aux)
    finally
        ccall((:lsm_render_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), r)
    end
end

# export_surface_mesh(ϕ, output) (ext/MMGSurfaceExt.jl:35-80) up to the remesher: the Medit .mesh file the reference hands to mmgs
# (_write_3D_triangular_mesh, :82-102), from the device's mesh.  The mmgs pass is not part of this library.
function LSM.export_surface_mesh(ϕ::ROCMeshField, output::String; level = 0.0, hgrad = nothing, hmin = nothing, hmax = nothing, hausd = nothing)
    ndims(ϕ) == 3 || throw(ArgumentError("export_mesh of $(ndims(ϕ)) dimensional level-set not supported."))
    all(isnothing, (hgrad, hmin, hmax, hausd)) ||
        error("export_surface_mesh: the mmgs remeshing pass is not part of this library; the file written without hgrad, hmin, hmax, hausd is its input")
    m = isosurface_arrays(ϕ; level)
    vertices, triangles = Array(m.vertices), Array(m.elements)
    open(output, "w") do io
        println(io, "MeshVersionFormatted 1\nDimension 3\n\nVertices\n", size(vertices, 2))
        foreach(v -> println(io, v[1], ' ', v[2], ' ', v[3], " 1"), eachcol(vertices))
        println(io, "\nTriangles\n", size(triangles, 2))
        foreach(t -> println(io, t[1] + 1, ' ', t[2] + 1, ' ', t[3] + 1, " 1"), eachcol(triangles))
        println(io, "\nEnd")
    end
    return output
end

# volume_mesh: the interior {ϕ < level} as a body-fitted simplicial mesh (include/lsm.h, lsm_vol_*): vertices ndim x nv, elements
# (ndim + 1) x ne (triangles in 2-D, tetrahedra in 3-D), interface ndim x ni (isosurface's elements), 0-based vertex numbers, all on
# the device.  Dense fields only: a band does not hold the interior.
function volume_mesh_arrays(ϕ::ROCMeshField; level = 0.0)
    out, c = Ref{Ptr{Cvoid}}(), zeros(Int64, 3)
    _check(ϕ.h.ptr, ccall((:lsm_vol_create, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ref{Ptr{Cvoid}}, Ptr{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), C_NULL, level, out, c), "lsm_vol_create")
    s = out[]
    try
        nv, ne, ni = c
        N = ndims(ϕ)
        vertices, elements, interface = ROCMatrix{Float64}(undef, N, nv), ROCMatrix{Int64}(undef, N + 1, ne), ROCMatrix{Int64}(undef, N, ni)
        _check(ϕ.h.ptr, ccall((:lsm_vol_read, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
            s, pointer(vertices), pointer(elements), pointer(interface)), "lsm_vol_read")
        return (; vertices, elements, interface)
    finally
        ccall((:lsm_vol_destroy, libhiplsm), Cvoid, (Ptr{Cvoid},), s)
    end
end

# export_volume_mesh(ϕ, output) (ext/MMGVolumeExt.jl) up to the remesher: the splitting of the grid's Kuhn triangulation along ϕ = level
# that mmg2d_O3 / mmg3d_O3 -ls starts with, as a Medit .mesh file.  References: vertices 1, elements 3 (the ϕ < 0 subdomain),
# interface 10.  The remeshing pass is not part of this library.
function LSM.export_volume_mesh(ϕ::ROCMeshField, output::String; level = 0.0, hgrad = nothing, hmin = nothing, hmax = nothing, hausd = nothing)
    N = ndims(ϕ)
    N in (2, 3) || throw(ArgumentError("export_mesh of $N dimensional level-set not supported."))
    all(isnothing, (hgrad, hmin, hmax, hausd)) ||
        error("export_volume_mesh: the mmg2d_O3 / mmg3d_O3 remeshing pass is not part of this library; the file written without hgrad, hmin, hmax, hausd is the splitting it starts from")
    m = volume_mesh_arrays(ϕ; level)
    vertices, elements, interface = Array(m.vertices), Array(m.elements), Array(m.interface)
    open(output, "w") do io
        println(io, "MeshVersionFormatted 1\nDimension ", N, "\n\nVertices\n", size(vertices, 2))
        foreach(v -> println(io, join(v, ' '), " 1"), eachcol(vertices))
        println(io, "\n", N == 2 ? "Triangles" : "Tetrahedra", "\n", size(elements, 2))
        foreach(t -> println(io, join(t .+ 1, ' '), " 3"), eachcol(elements))
        println(io, "\n", N == 2 ? "Edges" : "Triangles", "\n", size(interface, 2))
        foreach(t -> println(io, join(t .+ 1, ' '), " 10"), eachcol(interface))
        println(io, "\nEnd")
    end
    return output
end

# reinitialize!(ϕ; ...) (src/reinitializer.jl:12-42)
function LSM.reinitialize!(ϕ::ROCMeshField; order = 3, upsample = 2, maxiters = 20, xtol = nothing, ftol = nothing)
    xt, ft = something(xtol, sqrt(eps(Float64))), something(ftol, sqrt(eps(Float64)))
    _check(ϕ.h.ptr, ccall((:lsm_fill_ghosts, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}), ϕ.h.ptr, pointer(ϕ.buf), 7, C_NULL), "lsm_fill_ghosts")
    work = similar(ϕ.buf)
    nc, nfail, nfar = Ref{Int64}(), Ref{Int64}(), Ref{Int64}()
    _check(ϕ.h.ptr, ccall((:lsm_reinitialize, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Cint, Float64, Float64, Ref{Int64}, Ref{Int64}, Ref{Int64}),
        ϕ.h.ptr, pointer(ϕ.buf), C_NULL, pointer(work), order, upsample, maxiters, xt, ft, nc, nfail, nfar), "lsm_reinitialize")
    nfail[] > 0 && @warn "reinitialize!: closest-point solver did not converge for $(nfail[]) points"
    return ϕ
end

# ---- NarrowBandMeshField on the device (src/meshfield.jl:314-588): dense padded values + byte masks --------------------
# The reference steps a band field with the SAME _advance! / compute_cfl / update_band! sequence as a dense one
# (src/timestepping.jl:101-122,126-202; src/meshfield.jl:555-588); the methods below are that sequence for a device band.
const BAND_MC = 16            # planes per tile along the last dimension (8, 12, 16, 24, 32 measured at 768³: 16 is the fastest)
const BAND_OVERLAP = 10       # planes of each neighbouring rank a slab of a band holds (include/lsm.h, lsm_band_overlap_config)
mutable struct ROCNarrowBandMeshField{N, T, B, S} <: LSM.AbstractMeshField{N, T, S}
    buf::ROCVector{S}
    mesh::LSM.CartesianGrid{N, T}
    bcs::B
    h::Handle
    samples::Dict{UInt, Vector{ROCVector{Float64}}}
    nlayers::Int
    mask::ROCVector{UInt8}
    halo::ROCVector{UInt8}
    tiles::ROCVector{UInt8}
    scratch::NTuple{2, ROCVector{UInt8}}
    hlist::ROCVector{Int64}       # (halo node -> nearest band node) entries, 2 Int64 each
    hcount::ROCVector{UInt32}
    own::Tuple{Int, Int}          # (first local plane, count) of the planes this rank owns; the rest are overlap planes
end
const ROCField = Union{ROCMeshField, ROCNarrowBandMeshField}

function _tile_count(h::Handle)
    n = Ref{Int64}()
    _check(h.ptr, ccall((:lsm_band_tile_count, libhiplsm), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}), h.ptr, BAND_MC, n), "lsm_band_tile_count")
    return Int(n[])
end
function _empty_band(buf::ROCVector{S}, mesh::LSM.CartesianGrid{N, T}, bcs, h, nlayers, own) where {N, T, S}
    total = h.layout.total
    bytes() = AMDGPU.zeros(UInt8, total)
    return ROCNarrowBandMeshField{N, T, typeof(bcs), S}(buf, mesh, bcs, h, Dict{UInt, Vector{ROCVector{Float64}}}(), nlayers, bytes(), bytes(),
        AMDGPU.zeros(UInt8, _tile_count(h)), (bytes(), bytes()), ROCVector{Int64}(undef, 2 * (1 << 16)), AMDGPU.zeros(UInt32, 1), own)
end

# NarrowBandMeshField(ϕ; nlayers) (src/meshfield.jl:411-440) on the device.  slab = (lo, n, rank, world): the OWNED planes;
# the handle's slab is extended by BAND_OVERLAP planes of each neighbour (attach a communicator, then band_overlap!).
function ROCNarrowBandMeshField(nb::LSM.NarrowBandMeshField{N, T}; strict = false, slab = nothing) where {N, T}
    bcs = LSM.boundary_conditions(nb)
    any(bc -> bc isa LSM.PeriodicBC, Iterators.flatten(bcs)) && throw(ArgumentError("PeriodicBC is not supported on a NarrowBandMeshField"))
    dense = LSM.MeshField(nb)                      # every node: the band is re-derived on the device (from_dense)
    S = eltype(values(dense))
    ext, own = slab, (0, LSM.mesh(nb).n[N])
    if slab !== nothing
        lo, n, rank, world = slab
        wlo, whi = rank > 0 ? BAND_OVERLAP : 0, rank < world - 1 ? BAND_OVERLAP : 0
        ext, own = (lo - wlo, n + wlo + whi, rank, world), (wlo, n)
    end
    h = Handle(LSM.mesh(nb), bcs, S; strict, slab = ext)
    ϕ = _empty_band(AMDGPU.zeros(S, h.layout.total), LSM.mesh(nb), bcs, h, nb.nlayers, own)
    _check(h.ptr, ccall((:lsm_upload, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h.ptr, pointer(ϕ.buf), _local(values(dense), ext)), "lsm_upload")
    slab === nothing && LSM.update_band!(ϕ; from_dense = true)     # a slab builds its band in band_overlap!, once attached
    return ϕ
end
# after attach_rccl! / attach_local! on the band fields of all ranks: declare the overlap, build the band, take the overlap
# planes from their owners
function band_overlap!(ϕ::ROCNarrowBandMeshField)
    _check(ϕ.h.ptr, ccall((:lsm_band_overlap_config, libhiplsm), Cint, (Ptr{Cvoid}, Int64), ϕ.h.ptr, BAND_OVERLAP), "lsm_band_overlap_config")
    return LSM.update_band!(ϕ; from_dense = true)
end
attach_rccl!(ϕ::ROCNarrowBandMeshField, id::Vector{UInt8}) =
    (_check(ϕ.h.ptr, ccall((:lsm_comm_attach_rccl, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint), ϕ.h.ptr, id, ϕ.h.rank, ϕ.h.world), "lsm_comm_attach_rccl"); band_overlap!(ϕ))
# a rank whose hook threw: the other ranks' exchanges return LSM_ERR_COMM instead of waiting for it
comm_abort!(ϕ::ROCField) = _check(ϕ.h.ptr, ccall((:lsm_comm_abort, libhiplsm), Cint, (Ptr{Cvoid},), ϕ.h.ptr), "lsm_comm_abort")

# a copy shares the handle; the band set travels with it (the Dict copy of src/meshfield.jl:420-423)
function Base.copy(ϕ::ROCNarrowBandMeshField{N, T, B, S}) where {N, T, B, S}
    return ROCNarrowBandMeshField{N, T, B, S}(copy(ϕ.buf), ϕ.mesh, ϕ.bcs, ϕ.h, ϕ.samples, ϕ.nlayers, copy(ϕ.mask), copy(ϕ.halo), copy(ϕ.tiles),
        (similar(ϕ.mask), similar(ϕ.mask)), copy(ϕ.hlist), copy(ϕ.hcount), ϕ.own)
end
function Base.copy!(dst::ROCNarrowBandMeshField, src::ROCNarrowBandMeshField)      # src/meshfield.jl:282-292: values AND keys
    copyto!(dst.buf, src.buf); copyto!(dst.mask, src.mask); copyto!(dst.halo, src.halo); copyto!(dst.tiles, src.tiles)
    dst.hlist = copy(src.hlist); copyto!(dst.hcount, src.hcount)
    # the handle's compact tile lists, the halo list's length as the host knows it and a prefetched Δt describe the band these
    # buffers held BEFORE: rebuild them from the new contents (api.py's copy_ does the same; include/lsm.h, lsm_band_invalidate)
    _check(dst.h.ptr, ccall((:lsm_band_retile, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint), dst.h.ptr, pointer(dst.mask), pointer(dst.tiles), BAND_MC), "lsm_band_retile")
    _band_status(dst)
    return dst
end
function Base.values(ϕ::ROCNarrowBandMeshField{N, T, B, S}) where {N, T, B, S}
    out = Array{S, N}(undef, ntuple(d -> Int(ϕ.h.layout.n[d]), N))
    _check(ϕ.h.ptr, ccall((:lsm_download, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), ϕ.h.ptr, pointer(ϕ.buf), out), "lsm_download")
    return out
end

struct LsmBand
    mask::Ptr{Cvoid}
    tiles::Ptr{Cvoid}
    mc::Int32
    _pad::Int32
    halo_list::Ptr{Cvoid}
    halo_cap::Int64
    halo_count::Ptr{Cvoid}
end
_band(ϕ::ROCNarrowBandMeshField) = Ref(LsmBand(pointer(ϕ.mask), pointer(ϕ.tiles), BAND_MC, 0, pointer(ϕ.hlist), length(ϕ.hlist) ÷ 2, pointer(ϕ.hcount)))

function _band_status(ϕ::ROCNarrowBandMeshField)
    want, missed = Ref{Int64}(), Ref{Cint}()
    _check(ϕ.h.ptr, ccall((:lsm_band_status, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Ref{Cint}),
        ϕ.h.ptr, pointer(ϕ.hcount), want, missed), "lsm_band_status")
    missed[] != 0 && throw(ArgumentError("index is more than $(LSM._BAND_SEARCH_RADIUS) nodes from the band"))   # src/meshfield.jl:499-500
    return Int(want[])
end
_band_halo(ϕ::ROCNarrowBandMeshField) = _check(ϕ.h.ptr, ccall((:lsm_band_halo, libhiplsm), Cint,
    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
    ϕ.h.ptr, pointer(ϕ.buf), pointer(ϕ.mask), pointer(ϕ.halo), pointer(ϕ.tiles), BAND_MC, pointer(ϕ.hlist), length(ϕ.hlist) ÷ 2, pointer(ϕ.hcount)), "lsm_band_halo")

# update_band!(ϕ) (src/timestepping.jl:115, src/meshfield.jl:555-588)
function LSM.update_band!(ϕ::ROCNarrowBandMeshField; from_dense = false)
    _check(ϕ.h.ptr, ccall((:lsm_band_update, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
        ϕ.h.ptr, pointer(ϕ.buf), pointer(ϕ.mask), from_dense, ϕ.nlayers, pointer(ϕ.scratch[1]), pointer(ϕ.scratch[2]),
        pointer(ϕ.halo), pointer(ϕ.tiles), BAND_MC, pointer(ϕ.hlist), length(ϕ.hlist) ÷ 2, pointer(ϕ.hcount)), "lsm_band_update")
    want = _band_status(ϕ)
    if ϕ.h.world > 1
        # slab: band set and new values are right only away from the cut faces — the overlap planes come from their owners
        # (mask as whole planes, then only the band nodes' values), and tiles / lists / halo are re-derived from the full mask
        _check(ϕ.h.ptr, ccall((:lsm_band_overlap_mask, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ϕ.h.ptr, pointer(ϕ.mask)), "lsm_band_overlap_mask")
        _check(ϕ.h.ptr, ccall((:lsm_band_overlap_values, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), ϕ.h.ptr, pointer(ϕ.buf)), "lsm_band_overlap_values")
        _check(ϕ.h.ptr, ccall((:lsm_band_retile, libhiplsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint), ϕ.h.ptr, pointer(ϕ.mask), pointer(ϕ.tiles), BAND_MC), "lsm_band_retile")
        _band_status(ϕ)
        _band_halo(ϕ)
        want = _band_status(ϕ)
    end
    while want > length(ϕ.hlist) ÷ 2               # list too short: grow it, derive the halo again
        ϕ.hlist = ROCVector{Int64}(undef, 4 * want)
        _band_halo(ϕ)
        want = _band_status(ϕ)
    end
    return ϕ
end

function LSM.compute_cfl(terms, ϕ::ROCNarrowBandMeshField, t)
    ts = [_term(term, ϕ, t) for term in terms]
    dt = Ref{Float64}(0.0)
    _check(ϕ.h.ptr, ccall((:lsm_compute_cfl_band, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Ref{Float64}),
        ϕ.h.ptr, ts, length(ts), pointer(ϕ.buf), pointer(ϕ.mask), pointer(ϕ.tiles), BAND_MC, t, dt), "lsm_compute_cfl_band")
    ϕ.h.world > 1 && _check(ϕ.h.ptr, ccall((:lsm_allreduce_dt, libhiplsm), Cint, (Ptr{Cvoid}, Ref{Float64}), ϕ.h.ptr, dt), "lsm_allreduce_dt")
    Δt = dt[]
    Δt > 0 || throw(ArgumentError("invalid time-step based on CFL condition: Δt = $Δt (check for NaN/Inf in velocity or speed)"))
    return Δt
end

# buffers: value arrays only — their off-band entries are scratch, the band set is ϕ's (src/timestepping.jl:126,141,168 copy ϕ)
_value_buffer(ϕ::ROCNarrowBandMeshField{N, T, B, S}) where {N, T, B, S} = ROCMeshField{N, T, B, S}(similar(ϕ.buf), ϕ.mesh, ϕ.bcs, ϕ.h, ϕ.samples)
LSM._alloc_buffers(::LSM.ForwardEuler, ϕ::ROCNarrowBandMeshField) = (_value_buffer(ϕ),)
LSM._alloc_buffers(::Union{LSM.RK2, LSM.RK3}, ϕ::ROCNarrowBandMeshField) = (_value_buffer(ϕ), _value_buffer(ϕ))

# _advance! on a band (src/timestepping.jl:128-202 over active_nodeindices): lsm_advance_band_* prepares every stage input
# (band halo by affine extrapolation, src/meshfield.jl:481-511, then the boundary ghosts), runs the band-restricted stages and,
# on a slab, refreshes the overlap planes of every stage result
function LSM._advance!(::LSM.ForwardEuler, ϕ::ROCNarrowBandMeshField, (dst,), terms, tc, Δt)
    ts = [_term(term, ϕ, tc) for term in terms]
    hook, band = _hook(terms, (ϕ,)), _band(ϕ)
    GC.@preserve hook _check(ϕ.h.ptr, ccall((:lsm_advance_band_fe, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ref{LsmBand}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, ts, length(ts), band, pointer(ϕ.buf), pointer(dst.buf), tc, Δt, hook, C_NULL), "lsm_advance_band_fe")
    return ϕ
end
function LSM._advance!(::LSM.RK2, ϕ::ROCNarrowBandMeshField, (pred, corr), terms, tc, Δt)
    ts = [_term(term, ϕ, tc) for term in terms]
    hook, band = _hook(terms, (ϕ, pred)), _band(ϕ)
    GC.@preserve hook _check(ϕ.h.ptr, ccall((:lsm_advance_band_rk2, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ref{LsmBand}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, ts, length(ts), band, pointer(ϕ.buf), pointer(pred.buf), pointer(corr.buf), tc, Δt, hook, C_NULL), "lsm_advance_band_rk2")
    return ϕ
end
function LSM._advance!(::LSM.RK3, ϕ::ROCNarrowBandMeshField, (buf1, buf2), terms, tc, Δt)
    ts = [_term(term, ϕ, tc) for term in terms]
    hook, band = _hook(terms, (ϕ, buf1, buf2)), _band(ϕ)
    GC.@preserve hook _check(ϕ.h.ptr, ccall((:lsm_advance_band_rk3, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ref{LsmBand}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
        ϕ.h.ptr, ts, length(ts), band, pointer(ϕ.buf), pointer(buf1.buf), pointer(buf2.buf), tc, Δt, hook, C_NULL), "lsm_advance_band_rk3")
    return ϕ
end

# one stage by hand (a driver of its own): the stage input made readable by stencils, then the band-restricted stage
function _band_stage!(ϕ::ROCNarrowBandMeshField, ts, psi, phin, out, out2, mode, cdt, cdt2, t)
    _check(ϕ.h.ptr, ccall((:lsm_band_prepare, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Cint),
        ϕ.h.ptr, psi, pointer(ϕ.mask), pointer(ϕ.hlist), length(ϕ.hlist) ÷ 2, pointer(ϕ.hcount), pointer(ϕ.tiles), BAND_MC), "lsm_band_prepare")
    _check(ϕ.h.ptr, ccall((:lsm_stage_band, libhiplsm), Cint,
        (Ptr{Cvoid}, Ptr{LsmTerm}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
        ϕ.h.ptr, ts, length(ts), psi, phin, out, out2, mode, cdt, cdt2, t, pointer(ϕ.mask), pointer(ϕ.tiles), BAND_MC, C_NULL), "lsm_stage_band")
end

# usage (drop-in):
#   ϕ  = MeshField(x -> norm(x) - 0.5, grid; bc = NeumannBC())
#   eq = LevelSetEquation(; terms = (AdvectionTerm(RigidRotation(1.0, (0.0, 0.0))),), ic = ROCMeshField(ϕ), integrator = RK3())
#   integrate!(eq, 1.0)              # _integrate! (src/timestepping.jl:101-122) runs unchanged on the host
#   ϕ_final = MeshField(current_state(eq))

end # module
