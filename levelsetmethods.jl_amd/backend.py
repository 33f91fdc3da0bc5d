"""HipBackend — device memory (torch tensors as plain HBM buffers), streams and the calls into
libhiplsm.so.  torch is plumbing here: allocation, the current HIP stream, and — in slab mode — the bootstrap
of the library's own RCCL communicator (the ghost-plane exchange, the Δt all-reduce and the overlap planes of a
slab-decomposed narrow band all run inside the library).

The interface (layout / alloc / upload / download / fill_ghosts / stage / compute_cfl_local /
advance_single / eikonal_sign / extrema / table) is the seam the host logic in api.py talks to.
The only implementation in this package is the HIP one; it raises if the library or the GPU is
missing — there is no CPU path.
"""
import ctypes as C
import functools

import numpy as np

from . import _lib as L


class HipBackend:
    name = "hip"

    def __init__(self, grid_c, bc_c, slab=None, mode="fast", device=0, dtype=np.float64, tuning=None):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("levelsetmethods.jl_amd needs an AMD GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.torch = torch
        self.lib = L.lib()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.ndim = int(grid_c.ndim)
        self._grid = grid_c
        self._bc = bc_c
        self.slab = slab
        self.dtype = np.dtype(dtype)          # storage of the level-set fields (float64 | float32); side arrays are float64
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError(f"unsupported field dtype {self.dtype}: float64 or float32")
        h = C.c_void_p()
        slab_c = L.LsmSlab(slab[0], slab[1]) if slab is not None else None
        code = self.lib.lsm_create(C.byref(grid_c), bc_c, C.byref(slab_c) if slab_c is not None else None,
                                   L.DTYPE_F32 if self.dtype == np.float32 else L.DTYPE_F64,
                                   L.MODE_STRICT if mode == "strict" else L.MODE_FAST, device, C.byref(h))
        if code != L.OK:
            raise L.LsmError(f"lsm_create failed ({code}): {self.lib.lsm_last_error(None).decode()}")
        self.h = h
        # kernels, torch copies and RCCL all order on torch's current stream
        L.check(self.h, self.lib.lsm_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                "lsm_set_stream")
        self.lay = L.LsmLayout()
        L.check(self.h, self.lib.lsm_layout(self.h, C.byref(self.lay)), "lsm_layout")
        for name, value in (tuning or {}).items():     # include/lsm.h, "tuning switches": before anything is built on the handle
            self.set_tuning(name, value)

    def close(self):
        if getattr(self, "h", None):
            self.lib.lsm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- memory
    def alloc(self):
        """A level-set field (ϕ, stage buffer, extension target) in the handle's storage type."""
        tdt = self.torch.float32 if self.dtype == np.float32 else self.torch.float64
        return self.torch.zeros(int(self.lay.total), dtype=tdt, device=self.device)

    def alloc_side(self):
        """A side array (coefficient field, frozen sign / mask): always float64."""
        return self.torch.zeros(int(self.lay.total), dtype=self.torch.float64, device=self.device)

    def clone(self, t):
        return t.clone()

    def copy_(self, dst, src):
        dst.copy_(src)

    def ptr(self, t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def local_shape(self):
        return tuple(int(self.lay.n[d]) for d in range(self.ndim))

    def upload(self, t, dense):
        a = np.asfortranarray(dense, dtype=self.dtype)
        assert a.shape == self.local_shape(), (a.shape, self.local_shape())
        L.check(self.h, self.lib.lsm_upload(self.h, self.ptr(t), a.ctypes.data_as(C.c_void_p)), "lsm_upload")

    def download(self, t):
        out = np.empty(self.local_shape(), dtype=self.dtype, order="F")
        L.check(self.h, self.lib.lsm_download(self.h, self.ptr(t), out.ctypes.data_as(C.c_void_p)), "lsm_download")
        return out

    def upload_side(self, t, dense):
        a = np.asfortranarray(dense, dtype=np.float64)
        assert a.shape == self.local_shape(), (a.shape, self.local_shape())
        L.check(self.h, self.lib.lsm_upload_f64(self.h, self.ptr(t), a.ctypes.data_as(C.c_void_p)), "lsm_upload_f64")

    def download_side(self, t):
        out = np.empty(self.local_shape(), dtype=np.float64, order="F")
        L.check(self.h, self.lib.lsm_download_f64(self.h, self.ptr(t), out.ctypes.data_as(C.c_void_p)), "lsm_download_f64")
        return out

    def table(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).to(self.device)

    def flat(self, t):
        return t

    # ---- kernels
    def fill_ghosts(self, t, mask=7):
        L.check(self.h, self.lib.lsm_fill_ghosts(self.h, self.ptr(t), mask, None), "lsm_fill_ghosts")

    def stage(self, terms_c, nterms, psi, phin, out, out2, base_mode, cdt, cdt2, t):
        L.check(self.h, self.lib.lsm_stage(self.h, terms_c, nterms, self.ptr(psi), self.ptr(phin), self.ptr(out),
                                           self.ptr(out2), base_mode, cdt, cdt2, t, None), "lsm_stage")

    def stage_planes(self, terms_c, nterms, psi, phin, out, out2, base_mode, cdt, cdt2, t, m0, m1):
        L.check(self.h, self.lib.lsm_stage_planes(self.h, terms_c, nterms, self.ptr(psi), self.ptr(phin), self.ptr(out),
                                                  self.ptr(out2), base_mode, cdt, cdt2, t, m0, m1, None), "lsm_stage_planes")

    def fill_ghosts_planes(self, t, m0, m1, fill_last=False):
        L.check(self.h, self.lib.lsm_fill_ghosts_planes(self.h, self.ptr(t), m0, m1, 1 if fill_last else 0, None),
                "lsm_fill_ghosts_planes")

    def compute_cfl_local(self, terms_c, nterms, phi, t):
        dt = C.c_double(0.0)
        L.check(self.h, self.lib.lsm_compute_cfl(self.h, terms_c, nterms, self.ptr(phi), t, C.byref(dt)), "lsm_compute_cfl")
        return dt.value

    def cfl_cache(self, enable):
        L.check(self.h, self.lib.lsm_cfl_cache(self.h, 1 if enable else 0), "lsm_cfl_cache")

    def advance_single(self, which, terms_c, nterms, phi, b1, b2, tc, dt, hook):
        cb = hook if hook is not None else C.cast(None, L.StageHook)
        if which == "fe":
            code = self.lib.lsm_advance_fe(self.h, terms_c, nterms, self.ptr(phi), self.ptr(b1), tc, dt, cb, None)
        elif which == "rk2":
            code = self.lib.lsm_advance_rk2(self.h, terms_c, nterms, self.ptr(phi), self.ptr(b1), self.ptr(b2), tc, dt, cb, None)
        else:
            code = self.lib.lsm_advance_rk3(self.h, terms_c, nterms, self.ptr(phi), self.ptr(b1), self.ptr(b2), tc, dt, cb, None)
        L.check(self.h, code, f"lsm_advance_{which}")

    def advance_i2oe(self, term_c, phi, tc, dt, rtol, max_iters):
        """One SemiImplicitI2OE step (lsm_advance_i2oe); returns (iterations, ‖r‖₂/‖rhs‖₂)."""
        it, rel = C.c_int(0), C.c_double(0.0)
        L.check(self.h, self.lib.lsm_advance_i2oe(self.h, term_c, self.ptr(phi), tc, dt, rtol, max_iters, C.byref(it), C.byref(rel)),
                "lsm_advance_i2oe")
        return it.value, rel.value

    def advance_semilag(self, term_c, phi, out, tc, dt, order=3, trace=2, limiter=True, want_stats=True):
        """One SemiLagrangian step (lsm_advance_semilag), out of place: the interior of `out` is the new state.  Returns
        (staged workgroups, fallback workgroups, largest displacement in cells), or None without want_stats (no host wait)."""
        st = (C.c_int64 * 3)() if want_stats else None
        L.check(self.h, self.lib.lsm_advance_semilag(self.h, term_c, self.ptr(phi), self.ptr(out), tc, dt, order, trace, 1 if limiter else 0, st),
                "lsm_advance_semilag")
        return (int(st[0]), int(st[1]), int(st[2])) if want_stats else None

    def check_range(self, t):
        """(ok, max|ϕ|): is the field inside the domain of the handle's arithmetic mode (include/lsm.h, LSM_FAST_MAX_ABS)?"""
        ok, m = C.c_int(), C.c_double()
        L.check(self.h, self.lib.lsm_check_range(self.h, self.ptr(t), C.byref(ok), C.byref(m)), "lsm_check_range")
        return bool(ok.value), m.value

    # ---- multi-GPU: slab communicator inside the library (include/lsm.h, "multi-GPU")
    def comm_unique_id(self):
        buf = C.create_string_buffer(L.COMM_ID_BYTES)
        L.check(None, self.lib.lsm_comm_unique_id(buf), "lsm_comm_unique_id")
        return buf.raw

    def comm_attach_rccl(self, unique_id, rank, world):
        """Collective over the ranks: ncclCommInitRank on this handle's device."""
        L.check(self.h, self.lib.lsm_comm_attach_rccl(self.h, C.c_char_p(unique_id), rank, world), "lsm_comm_attach_rccl")

    @staticmethod
    def comm_attach_local(backends):
        """All ranks in this process: backends[r] = rank r (LSM_COMM_LOCAL)."""
        arr = (C.c_void_p * len(backends))(*[b.h for b in backends])
        code = backends[0].lib.lsm_comm_attach_local(arr, len(backends))
        if code != L.OK:
            msgs = [b.lib.lsm_last_error(b.h) for b in backends]
            raise L.LsmError(f"lsm_comm_attach_local failed ({code}): " + "; ".join(m.decode() for m in msgs if m))

    def comm_detach(self):
        L.check(self.h, self.lib.lsm_comm_detach(self.h), "lsm_comm_detach")

    def comm_info(self):
        r, w, t = C.c_int(), C.c_int(), C.c_int()
        L.check(self.h, self.lib.lsm_comm_info(self.h, C.byref(r), C.byref(w), C.byref(t)), "lsm_comm_info")
        return r.value, w.value, t.value

    def comm_set_overlap(self, enable):
        L.check(self.h, self.lib.lsm_comm_set_overlap(self.h, 1 if enable else 0), "lsm_comm_set_overlap")

    def halo_start(self, t):
        L.check(self.h, self.lib.lsm_halo_start(self.h, self.ptr(t)), "lsm_halo_start")

    def halo_wait(self):
        L.check(self.h, self.lib.lsm_halo_wait(self.h), "lsm_halo_wait")

    def halo_exchange(self, t):
        L.check(self.h, self.lib.lsm_halo_exchange(self.h, self.ptr(t)), "lsm_halo_exchange")

    def allreduce_dt(self, dt):
        v = C.c_double(dt)
        L.check(self.h, self.lib.lsm_allreduce_dt(self.h, C.byref(v)), "lsm_allreduce_dt")
        return v.value

    def comm_abort(self):
        """Fail this rank's communicator (LOCAL: the whole group): peers blocked in an exchange get LSM_ERR_COMM."""
        if getattr(self, "h", None):
            self.lib.lsm_comm_abort(self.h)

    def band_overlap_config(self, overlap):
        L.check(self.h, self.lib.lsm_band_overlap_config(self.h, int(overlap)), "lsm_band_overlap_config")

    def band_overlap_mask(self, mask):
        L.check(self.h, self.lib.lsm_band_overlap_mask(self.h, self.ptr(mask)), "lsm_band_overlap_mask")

    def band_overlap_values(self, t):
        L.check(self.h, self.lib.lsm_band_overlap_values(self.h, self.ptr(t)), "lsm_band_overlap_values")

    def eikonal_sign(self, phi0, s0):
        L.check(self.h, self.lib.lsm_eikonal_sign(self.h, self.ptr(phi0), self.ptr(s0), None), "lsm_eikonal_sign")

    def extrema(self, t):
        lo, hi = C.c_double(), C.c_double()
        L.check(self.h, self.lib.lsm_extrema(self.h, self.ptr(t), C.byref(lo), C.byref(hi)), "lsm_extrema")
        return lo.value, hi.value

    def geometry(self, what, phi, outs, scale=1.0, band_width=-1.0, fill=0.0, frozen_out=None, mask=None):
        """curvature / gradient / normal of phi at every node (mask: at the band nodes of a prepared band field) into
        fp64 side arrays (lsm_geometry / lsm_band_geometry)."""
        o = [self.ptr(t) for t in outs] + [None] * (3 - len(outs))
        if mask is None:
            L.check(self.h, self.lib.lsm_geometry(self.h, int(what), self.ptr(phi), float(scale), float(band_width), float(fill), o[0], o[1], o[2],
                                                  self.ptr(frozen_out), None), "lsm_geometry")
        else:
            L.check(self.h, self.lib.lsm_band_geometry(self.h, int(what), self.ptr(phi), self.ptr(mask), float(scale), float(band_width), float(fill),
                                                       o[0], o[1], o[2], self.ptr(frozen_out), None), "lsm_band_geometry")

    def interpolate(self, phi, order, pts, want_grad, want_hess):
        """InterpolatedField evaluation at host points (npts x ndim): returns (values, gradients or None, hessians or None)."""
        t = self.torch
        p = t.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(self.device)
        n, N = int(p.shape[0]), self.ndim
        val = t.empty(n, dtype=t.float64, device=self.device)
        grad = t.empty((n, N), dtype=t.float64, device=self.device) if want_grad else None
        hess = t.empty((n, N, N), dtype=t.float64, device=self.device) if want_hess else None
        L.check(self.h, self.lib.lsm_interpolate(self.h, self.ptr(phi), int(order), n, self.ptr(p), self.ptr(val), self.ptr(grad), self.ptr(hess), None),
                "lsm_interpolate")
        self.sync()
        return val.cpu().numpy(), (grad.cpu().numpy() if want_grad else None), (hess.cpu().numpy() if want_hess else None)

    # ---- NewtonSDF objects (lsm_sdf_*)
    def sdf_create(self, phi, mask, order, upsample, maxiters, xtol, ftol):
        out, ns = C.c_void_p(), C.c_int64()
        L.check(self.h, self.lib.lsm_sdf_create(self.h, self.ptr(phi), self.ptr(mask), int(order), int(upsample), int(maxiters), float(xtol), float(ftol),
                                                C.byref(out), C.byref(ns)), "lsm_sdf_create")
        return out, int(ns.value)

    def sdf_eval(self, sdf, pts, want_cp):
        t = self.torch
        p = t.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(self.device)
        n, N = int(p.shape[0]), self.ndim
        dist = t.empty(n, dtype=t.float64, device=self.device)
        cp = t.empty((n, N), dtype=t.float64, device=self.device) if want_cp else None
        nf = C.c_int64()
        L.check(self.h, self.lib.lsm_sdf_eval(sdf, n, self.ptr(p), self.ptr(dist), self.ptr(cp), C.byref(nf)), "lsm_sdf_eval")
        return dist.cpu().numpy(), (cp.cpu().numpy() if want_cp else None), int(nf.value)

    def sdf_samples(self, sdf, nsamples):
        out = self.torch.empty((max(nsamples, 1), self.ndim), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_sdf_samples(sdf, self.ptr(out)), "lsm_sdf_samples")
        return out[:nsamples].cpu().numpy()

    def sdf_destroy(self, sdf):
        self.lib.lsm_sdf_destroy(sdf)

    # ---- quadrature results (lsm_quad_*)
    def quad_create(self, phi, mask, interpolation_order, quadrature_order, surface):
        """returns (result handle, (ncut, nnodes, nfull, nfallback))"""
        out, cnt = C.c_void_p(), (C.c_int64 * 4)()
        L.check(self.h, self.lib.lsm_quad_create(self.h, self.ptr(phi), self.ptr(mask), int(interpolation_order), int(quadrature_order),
                                                 int(bool(surface)), C.byref(out), cnt), "lsm_quad_create")
        return out, tuple(int(v) for v in cnt)

    def quad_read(self, quad, counts, q):
        """the result's device arrays: cells, offsets, coords, weights, full cells, rule coords, rule weights"""
        t, N = self.torch, self.ndim
        ncut, nnodes, nfull, _ = counts
        i64 = dict(dtype=t.int64, device=self.device)
        f64 = dict(dtype=t.float64, device=self.device)
        cells, offsets, full = t.empty(ncut, **i64), t.empty(ncut + 1, **i64), t.empty(nfull, **i64)
        coords, weights = t.empty((nnodes, N), **f64), t.empty(nnodes, **f64)
        rule_x, rule_w = t.empty((q ** N, N), **f64), t.empty(q ** N, **f64)
        L.check(self.h, self.lib.lsm_quad_read(quad, self.ptr(cells), self.ptr(offsets), self.ptr(coords), self.ptr(weights), self.ptr(full),
                                               self.ptr(rule_x), self.ptr(rule_w)), "lsm_quad_read")
        return cells, offsets, coords, weights, full, rule_x, rule_w

    def quad_total(self, quad):
        out = C.c_double()
        L.check(self.h, self.lib.lsm_quad_total(quad, C.byref(out)), "lsm_quad_total")
        return float(out.value)

    def quad_destroy(self, quad):
        self.lib.lsm_quad_destroy(quad)

    # ---- interface meshes (lsm_iso_*)
    def iso_create(self, phi, mask, level):
        """returns (result handle, (vertices, elements))"""
        out, cnt = C.c_void_p(), (C.c_int64 * 2)()
        L.check(self.h, self.lib.lsm_iso_create(self.h, self.ptr(phi), self.ptr(mask), float(level), C.byref(out), cnt), "lsm_iso_create")
        return out, tuple(int(v) for v in cnt)

    def iso_read(self, iso, counts):
        """the result's device arrays: vertices (nv, N) float64, elements (ne, N) int64"""
        t, N = self.torch, self.ndim
        nv, ne = counts
        verts = t.empty((nv, N), dtype=t.float64, device=self.device)
        elems = t.empty((ne, N), dtype=t.int64, device=self.device)
        L.check(self.h, self.lib.lsm_iso_read(iso, self.ptr(verts), self.ptr(elems)), "lsm_iso_read")
        return verts, elems

    def iso_destroy(self, iso):
        self.lib.lsm_iso_destroy(iso)

    # ---- from a mesh back to a level set (lsm_mesh_distance)
    def mesh_distance(self, phi, vertices, elements, cutoff):
        """ϕ := signed distance to the mesh, cut off; vertices (nv, N) float64 and elements (ne, N) int64 on the host or the
        device.  Returns (nodes with d < cutoff, unbalanced grid rows, elements the sign pass skipped)."""
        t = self.torch
        if getattr(self, "slab", None) is not None:
            raise L.LsmError("mesh_distance: this backend holds a slab of a decomposed grid; lsm_mesh_distance works on the whole grid of one device")
        if not t.is_tensor(vertices):
            vertices = np.array(vertices, dtype=np.float64, order="C")     # a copy torch may wrap (the caller's may be read-only)
        if not t.is_tensor(elements):
            elements = np.array(elements, dtype=np.int64, order="C")
        v = t.as_tensor(vertices, dtype=t.float64, device=self.device).contiguous()
        e = t.as_tensor(elements, dtype=t.int64, device=self.device).contiguous()
        stats = (C.c_int64 * 3)()
        L.check(self.h, self.lib.lsm_mesh_distance(self.h, int(v.shape[0]), self.ptr(v) if v.numel() else None, int(e.shape[0]),
                                                   self.ptr(e) if e.numel() else None, float(cutoff), self.ptr(phi), stats, None),
                "lsm_mesh_distance")
        return tuple(int(s) for s in stats)

    # ---- far-field distance and travel times (lsm_eikonal)
    def eikonal(self, phi, speed, width, cutoff, max_iters):
        """ϕ := copysign(min(T, cutoff), ϕ), |∇T| = 1/speed; speed: None or an n-shaped array of float64 (host or device), axis 0
        fastest; width 0: the crossing seed.  Returns (frozen nodes, outer iterations, tile visits, nodes clamped at the cutoff).  An
        LsmError raised for the data carries `reason`: 1 a non-finite ϕ, 2 a speed that is not finite and positive, 3 no interface."""
        t = self.torch
        if getattr(self, "slab", None) is not None:
            raise L.LsmError("eikonal: this backend holds a slab of a decomposed grid; lsm_eikonal works on the whole grid of one device")
        sp = None
        if speed is not None:
            if not t.is_tensor(speed):
                speed = np.array(speed, dtype=np.float64, order="F")            # a copy torch may wrap
                if speed.shape != self.local_shape():
                    raise L.LsmError(f"eikonal: the speed has shape {speed.shape}, the grid {self.local_shape()}")
                speed = speed.reshape(-1, order="F")
            sp = t.as_tensor(speed, dtype=t.float64, device=self.device).contiguous()
            if sp.numel() != int(np.prod(self.local_shape())):
                raise L.LsmError(f"eikonal: the speed has {sp.numel()} values, the grid {int(np.prod(self.local_shape()))} nodes")
        stats = (C.c_int64 * 4)()
        code = self.lib.lsm_eikonal(self.h, self.ptr(phi), self.ptr(sp) if sp is not None else None, float(width), float(cutoff),
                                    int(max_iters), stats, None)
        try:
            L.check(self.h, code, "lsm_eikonal")
        except L.LsmError as e:
            e.reason = -int(stats[0]) if code == L.ERR_INVALID and stats[0] < 0 else 0     # include/lsm.h: what the data was refused for
            raise
        return tuple(int(s) for s in stats)

    # ---- extension off a frozen set along the characteristics of |ϕ| (lsm_extend)
    EXTEND_RULES = {"rule": 0, "mask": 1, "inside": 2, "outside": 3}
    EXTEND_SOURCES = {"nodes": 0, "interface": 1}

    def extend(self, fields, phi, rule="rule", mask=None, width=0.0, source="nodes", cutoff=float("inf"), fill=0.0, max_iters=0):
        """fields: 1…8 device buffers of this backend, updated in place; rule: "rule", "mask" (mask: n-shaped, non-zero = frozen,
        host or device, axis 0 fastest), "inside" or "outside"; source: "nodes" or "interface"; width 0: the crossing seed.  Returns
        (frozen nodes, outer iterations, tile visits, orphans, filled nodes).  An LsmError raised for the data carries `reason`:
        1 a non-finite ϕ, 2 a non-finite field at a frozen node, 3 no frozen node."""
        t = self.torch
        if getattr(self, "slab", None) is not None:
            raise L.LsmError("extend: this backend holds a slab of a decomposed grid; lsm_extend works on the whole grid of one device")
        fields = list(fields)
        m = None
        if mask is not None:
            if not t.is_tensor(mask):
                mask = np.asarray(mask)
                if mask.shape != self.local_shape():
                    raise L.LsmError(f"extend: the mask has shape {mask.shape}, the grid {self.local_shape()}")
                mask = np.ascontiguousarray((mask != 0).reshape(-1, order="F").astype(np.uint8))
            m = t.as_tensor(mask, device=self.device).to(t.uint8).contiguous()
            if m.numel() != int(np.prod(self.local_shape())):
                raise L.LsmError(f"extend: the mask has {m.numel()} values, the grid {int(np.prod(self.local_shape()))} nodes")
        ptrs = (C.c_void_p * max(1, len(fields)))(*[self.ptr(f) for f in fields])
        stats = (C.c_int64 * 5)()
        code = self.lib.lsm_extend(self.h, self.ptr(phi), ptrs, len(fields), self.EXTEND_RULES[rule], self.ptr(m) if m is not None else None,
                                   float(width), self.EXTEND_SOURCES[source], float(cutoff), float(fill), int(max_iters), stats, None)
        try:
            L.check(self.h, code, "lsm_extend")
        except L.LsmError as e:
            e.reason = -int(stats[0]) if code == L.ERR_INVALID and stats[0] < 0 else 0     # include/lsm.h: what the data was refused for
            e.offenders = int(stats[1]) if e.reason else 0
            raise
        return tuple(int(s) for s in stats)

    # ---- connected components (lsm_cc_*)
    def cc_create(self, phi, level, side):
        """returns (result handle, (K, nodes in the set, cross-tile edges, non-finite nodes)); side 0: {ϕ < level}, 1: the
        complement.  An LsmError raised for a non-finite ϕ carries `nonfinite`, the number of such nodes."""
        if not self.torch.is_tensor(phi) or not phi.is_cuda:
            raise TypeError(f"cc_create takes a device buffer of this backend, not {type(phi).__name__}")
        if self.slab is not None:     # a one-rank group's slab is the whole grid with no communicator: the library could not tell
            raise L.LsmError("cc_create: this backend holds a slab of a decomposed grid; lsm_cc_create works on the whole grid of one device")
        out, stats = C.c_void_p(), (C.c_int64 * 4)()
        code = self.lib.lsm_cc_create(self.h, self.ptr(phi), float(level), int(side), C.byref(out), stats)
        try:
            L.check(self.h, code, "lsm_cc_create")
        except L.LsmError as e:
            e.nonfinite = int(stats[3]) if code == L.ERR_INVALID else 0
            raise
        return out, tuple(int(s) for s in stats)

    def cc_read(self, cc, K):
        """the result's device arrays: labels int32 (one per node, axis 0 fastest), nodes int64 (K), index sums int64 (K, N),
        bounding boxes int32 (K, 2, N)"""
        t, N = self.torch, self.ndim
        labels = t.empty(int(np.prod(self.local_shape())), dtype=t.int32, device=self.device)
        nodes = t.empty((K,), dtype=t.int64, device=self.device)
        sums = t.empty((K, N), dtype=t.int64, device=self.device)
        bbox = t.empty((K, 2, N), dtype=t.int32, device=self.device)
        L.check(self.h, self.lib.lsm_cc_read(cc, self.ptr(labels), self.ptr(nodes) if K else None, self.ptr(sums) if K else None,
                                             self.ptr(bbox) if K else None), "lsm_cc_read")
        return labels, nodes, sums, bbox

    def cc_flip(self, cc, phi, which):
        """flip the components flagged in `which` (a uint8 device tensor of K entries) in ϕ; returns the number of nodes written"""
        n = C.c_int64(0)
        L.check(self.h, self.lib.lsm_cc_flip(cc, self.ptr(phi), self.ptr(which), C.byref(n)), "lsm_cc_flip")
        return int(n.value)

    def cc_destroy(self, cc):
        self.lib.lsm_cc_destroy(cc)

    # ---- nucleation (lsm_nucleate_*)
    def nucleate_find(self, phi, t, threshold, level, clearance, spacing):
        """(linear indices int64, values fp64) of the centres, on the host, in ascending index"""
        for x in (phi, t):
            if not self.torch.is_tensor(x) or not x.is_cuda:
                raise TypeError(f"nucleate_find takes device buffers of this backend, not {type(x).__name__}")
        if self.slab is not None:     # a one-rank group's slab is the whole grid with no communicator: the library could not tell
            raise L.LsmError("nucleate_find: this backend holds a slab of a decomposed grid; lsm_nucleate_create works on the whole grid of one device")
        out, count = C.c_void_p(), C.c_int64(0)
        L.check(self.h, self.lib.lsm_nucleate_create(self.h, self.ptr(phi), self.ptr(t), float(threshold), float(level), float(clearance), float(spacing),
                                                     C.byref(out), C.byref(count)), "lsm_nucleate_create")
        try:
            K, tt = int(count.value), self.torch
            idx = tt.empty((K,), dtype=tt.int64, device=self.device)
            val = tt.empty((K,), dtype=tt.float64, device=self.device)
            if K:
                L.check(self.h, self.lib.lsm_nucleate_read(out, self.ptr(idx), self.ptr(val)), "lsm_nucleate_read")
            return idx.cpu().numpy(), val.cpu().numpy()
        finally:
            self.lib.lsm_nucleate_destroy(out)

    def nucleate_punch(self, phi, centres, level, radius):
        """punch balls around the linear node indices `centres` (host int64) into ϕ; returns the number of nodes changed"""
        if self.slab is not None:
            raise L.LsmError("nucleate_punch: this backend holds a slab of a decomposed grid; lsm_nucleate_punch works on the whole grid of one device")
        c = self.torch.from_numpy(np.ascontiguousarray(centres, dtype=np.int64)).to(self.device)
        n = C.c_int64(0)
        L.check(self.h, self.lib.lsm_nucleate_punch(self.h, self.ptr(phi), self.ptr(c) if c.numel() else None, int(c.numel()), float(level), float(radius),
                                                    C.byref(n)), "lsm_nucleate_punch")
        return int(n.value)

    # ---- elliptic solves (lsm_elliptic_*)
    def interior(self, t):
        """the interior of a padded field as a strided view, the grid's axes reversed (its C order is the grid's axis-0-fastest order)"""
        N = self.ndim
        return t.as_strided([int(self.lay.n[d]) for d in reversed(range(N))], [int(self.lay.stride[d]) for d in reversed(range(N))], int(self.lay.origin))

    def node_array(self, v, what, shape=None):
        """a flat float64 device array, axis 0 fastest, of the grid's shape (or `shape`): from a scalar, a host array or a device tensor"""
        t = self.torch
        shape = tuple(self.local_shape()) if shape is None else tuple(shape)
        count = int(np.prod(shape))
        if t.is_tensor(v):
            out = v.to(device=self.device, dtype=t.float64).contiguous().reshape(-1)
        elif np.ndim(v) == 0:
            out = t.full((count,), float(v), dtype=t.float64, device=self.device)
        else:
            a = np.asarray(v, dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"{what} has shape {a.shape}, expected {shape}")
            out = t.from_numpy(np.array(a.reshape(-1, order="F"))).to(self.device)
        if out.numel() != count:
            raise ValueError(f"{what} has {out.numel()} values, expected {count}")
        return out

    def elliptic_create(self, phi, level, a_in, a_out, a_cells, c_const, c_nodes, fixed, precond):
        """returns (object, (levels, free nodes, fixed nodes, 0)).  An LsmError raised for the data carries `reason` (include/lsm.h)."""
        if self.slab is not None:
            raise L.LsmError("elliptic_create: this backend holds a slab of a decomposed grid; lsm_elliptic_create works on the whole grid of one device")
        out, stats = C.c_void_p(), (C.c_int64 * 4)()
        code = self.lib.lsm_elliptic_create(self.h, self.ptr(phi), float(level), float(a_in), float(a_out), self.ptr(a_cells), float(c_const),
                                            self.ptr(c_nodes), self.ptr(fixed), int(precond), C.byref(out), stats)
        try:
            L.check(self.h, code, "lsm_elliptic_create")
        except L.LsmError as e:
            e.reason = -int(stats[0]) if code == L.ERR_INVALID and stats[0] < 0 else 0
            raise
        return out, tuple(int(v) for v in stats)

    def elliptic_apply(self, obj, x):
        y = self.torch.empty_like(x)
        L.check(self.h, self.lib.lsm_elliptic_apply(obj, self.ptr(x), self.ptr(y)), "lsm_elliptic_apply")
        return y

    def elliptic_solve(self, obj, f, u, rtol, max_iters):
        it, rel = C.c_int(0), C.c_double(0.0)
        L.check(self.h, self.lib.lsm_elliptic_solve(obj, self.ptr(f), self.ptr(u), float(rtol), int(max_iters), C.byref(it), C.byref(rel), None),
                "lsm_elliptic_solve")
        return it.value, rel.value

    def elliptic_energy(self, obj, u, e):
        L.check(self.h, self.lib.lsm_elliptic_energy(obj, self.ptr(u), self.ptr(e)), "lsm_elliptic_energy")

    def elliptic_compliance(self, obj, f, u):
        out = C.c_double(0.0)
        L.check(self.h, self.lib.lsm_elliptic_compliance(obj, self.ptr(f), self.ptr(u), C.byref(out)), "lsm_elliptic_compliance")
        return out.value

    def elliptic_cells(self, obj):
        n = self.local_shape()
        out = self.torch.empty(int(np.prod([m - 1 for m in n])), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elliptic_cells(obj, self.ptr(out)), "lsm_elliptic_cells")
        return out

    ELLIPTIC_MAXCOLS = 8

    def _fields_array(self, us):
        """the field pointers of K columns as a C array"""
        ptrs = [int(u.data_ptr()) for u in us]
        return (C.c_void_p * len(ptrs))(*ptrs)

    def elliptic_solve_many(self, obj, f, us, rtol, max_iters):
        """K columns in one batched solve: f the K·nn sources, us the K fields.  Returns (iterations, relres, status) tuples; raises after
        setting .iterations, .relres, .status on the error when the library filled them"""
        K = len(us)
        it, rel, stat = (C.c_int * K)(), (C.c_double * K)(), (C.c_int * K)()
        code = self.lib.lsm_elliptic_solve_many(obj, K, self.ptr(f), self._fields_array(us), float(rtol), int(max_iters), it, rel, stat, None)
        out = tuple(int(v) for v in it), tuple(float(v) for v in rel), tuple(int(v) for v in stat)
        if code != L.OK:
            try:
                L.check(self.h, code, "lsm_elliptic_solve_many")
            except L.LsmError as e:
                e.iterations, e.relres, e.status = out
                raise
        return out

    def elliptic_energy_many(self, obj, us, w, e):
        K = len(us)
        L.check(self.h, self.lib.lsm_elliptic_energy_many(obj, K, self._fields_array(us), (C.c_double * K)(*[float(v) for v in w]), self.ptr(e)),
                "lsm_elliptic_energy_many")

    def elliptic_energy_mutual(self, obj, u, v, e):
        L.check(self.h, self.lib.lsm_elliptic_energy_mutual(obj, self.ptr(u), self.ptr(v), self.ptr(e)), "lsm_elliptic_energy_mutual")

    def elliptic_destroy(self, obj):
        self.lib.lsm_elliptic_destroy(obj)

    # ---- elasticity solves (lsm_elastic_*): u is a tuple of N padded fields
    def _u3(self, u):
        return [self.ptr(t) for t in u] + [None] * (3 - len(u))

    def elastic_create(self, phi, level, e_in, e_out, e_cells, nu, plane, fixed, precond):
        """returns (object, (levels, free components, fixed components, 0)).  An LsmError raised for the data carries `reason` and
        `detail` (include/lsm.h)."""
        if self.slab is not None:
            raise L.LsmError("elastic_create: this backend holds a slab of a decomposed grid; lsm_elastic_create works on the whole grid of one device")
        out, stats = C.c_void_p(), (C.c_int64 * 4)()
        code = self.lib.lsm_elastic_create(self.h, self.ptr(phi), float(level), float(e_in), float(e_out), self.ptr(e_cells), float(nu), int(plane),
                                           self.ptr(fixed), int(precond), C.byref(out), stats)
        try:
            L.check(self.h, code, "lsm_elastic_create")
        except L.LsmError as e:
            e.reason = -int(stats[0]) if code == L.ERR_INVALID and stats[0] < 0 else 0
            e.detail = int(stats[1])
            raise
        return out, tuple(int(v) for v in stats)

    def elastic_stiffness(self, obj, level):
        R = (1 << self.ndim) * self.ndim
        out = np.zeros((R, R), dtype=np.float64)
        L.check(self.h, self.lib.lsm_elastic_stiffness(obj, int(level), out.ctypes.data_as(C.POINTER(C.c_double))), "lsm_elastic_stiffness")
        return out

    def elastic_apply(self, obj, x):
        y = self.torch.empty_like(x)
        L.check(self.h, self.lib.lsm_elastic_apply(obj, self.ptr(x), self.ptr(y)), "lsm_elastic_apply")
        return y

    def elastic_solve(self, obj, f, u, rtol, max_iters):
        it, rel = C.c_int(0), C.c_double(0.0)
        L.check(self.h, self.lib.lsm_elastic_solve(obj, self.ptr(f), *self._u3(u), float(rtol), int(max_iters), C.byref(it), C.byref(rel), None),
                "lsm_elastic_solve")
        return it.value, rel.value

    def elastic_energy(self, obj, u, e):
        L.check(self.h, self.lib.lsm_elastic_energy(obj, *self._u3(u), self.ptr(e)), "lsm_elastic_energy")

    def elastic_compliance(self, obj, f, u):
        out = C.c_double(0.0)
        L.check(self.h, self.lib.lsm_elastic_compliance(obj, self.ptr(f), *self._u3(u), C.byref(out)), "lsm_elastic_compliance")
        return out.value

    ELASTIC_MAXCOLS = 8

    def _ucols(self, us):
        """the K·N field pointers of K columns of N fields as a C array"""
        ptrs = [int(c.data_ptr()) for u in us for c in u]
        return (C.c_void_p * len(ptrs))(*ptrs)

    def elastic_solve_many(self, obj, f, us, rtol, max_iters):
        """K columns in one batched solve: f the K·N·nn loads, us K lists of N fields.  Returns (iterations, relres, status) tuples; raises
        after setting .iterations, .relres, .status on the error when the library filled them"""
        K = len(us)
        it, rel, stat = (C.c_int * K)(), (C.c_double * K)(), (C.c_int * K)()
        code = self.lib.lsm_elastic_solve_many(obj, K, self.ptr(f), self._ucols(us), float(rtol), int(max_iters), it, rel, stat, None)
        out = tuple(int(v) for v in it), tuple(float(v) for v in rel), tuple(int(v) for v in stat)
        if code != L.OK:
            try:
                L.check(self.h, code, "lsm_elastic_solve_many")
            except L.LsmError as e:
                e.iterations, e.relres, e.status = out
                raise
        return out

    def elastic_energy_many(self, obj, us, w, e):
        K = len(us)
        L.check(self.h, self.lib.lsm_elastic_energy_many(obj, K, self._ucols(us), (C.c_double * K)(*[float(v) for v in w]), self.ptr(e)), "lsm_elastic_energy_many")

    def elastic_energy_mutual(self, obj, u, v, e):
        L.check(self.h, self.lib.lsm_elastic_energy_mutual(obj, *self._u3(u), *self._u3(v), self.ptr(e)), "lsm_elastic_energy_mutual")

    def elastic_cells(self, obj):
        n = self.local_shape()
        out = self.torch.empty(int(np.prod([m - 1 for m in n])), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_cells(obj, self.ptr(out)), "lsm_elastic_cells")
        return out

    def elastic_destroy(self, obj):
        self.lib.lsm_elastic_destroy(obj)

    # ---- the periodic cell problems: homogenisation (lsm_homog_*) and conductivity homogenisation (lsm_hcond_*), csrc/cell_problem.h.
    # Vectors are flat float64 device tensors over the torus of n − 1 nodes per axis.  The methods homog_NAME and hcond_NAME are the
    # _cp_NAME below with the prefix bound (after the class).
    def _cp_sizes(self, pre):
        """(components per node, cell problems, nodes of the torus)"""
        N, nn = self.ndim, int(np.prod([m - 1 for m in self.local_shape()]))
        return (N, N * (N + 1) // 2, nn) if pre == "homog" else (1, N, nn)

    def _cp_check(self, pre, name, *args):
        fn = f"lsm_{pre}_{name}"
        L.check(self.h, getattr(self.lib, fn)(*args), fn)

    def _cp_device(self, pre, name, size, obj, *args):
        """the entry point's output, `size` doubles on the device"""
        out = self.torch.empty(size, dtype=self.torch.float64, device=self.device)
        self._cp_check(pre, name, obj, *args, self.ptr(out))
        return out

    def _cp_create(self, pre, phi, level, v_in, v_out, cells, *own):
        """own: the operator's own arguments, then the preconditioner.  Returns (object, (levels, free components, nodes of the torus,
        0)); an LsmError raised for the data carries `reason` and `detail`"""
        if self.slab is not None:
            raise L.LsmError(f"{pre}_create: this backend holds a slab of a decomposed grid; lsm_{pre}_create works on the whole grid of one device")
        out, stats = C.c_void_p(), (C.c_int64 * 4)()
        code = getattr(self.lib, f"lsm_{pre}_create")(self.h, self.ptr(phi), float(level), float(v_in), float(v_out), self.ptr(cells), *own, C.byref(out), stats)
        try:
            L.check(self.h, code, f"lsm_{pre}_create")
        except L.LsmError as e:
            e.reason = -int(stats[0]) if code == L.ERR_INVALID and stats[0] < 0 else 0
            e.detail = int(stats[1])
            raise
        return out, tuple(int(v) for v in stats)

    def _cp_cells(self, pre, obj):
        return self._cp_device(pre, "cells", self._cp_sizes(pre)[2], obj)

    def _cp_apply(self, pre, obj, x):
        y = self.torch.empty_like(x)
        self._cp_check(pre, "apply", obj, self.ptr(x), self.ptr(y))
        return y

    def _cp_load(self, pre, obj, k):
        nc, _, nn = self._cp_sizes(pre)
        return self._cp_device(pre, "load", nc * nn, obj, int(k))

    def _cp_solve(self, pre, obj, guess, rtol, max_iters):
        """guess: a flat float64 device tensor of all correctors or None; returns (iterations, relres), one entry per corrector"""
        K = self._cp_sizes(pre)[1]
        it, rel = (C.c_int * K)(), (C.c_double * K)()
        self._cp_check(pre, "solve", obj, self.ptr(guess), float(rtol), int(max_iters), it, rel)
        return [int(v) for v in it], [float(v) for v in rel]

    def _cp_solve_rhs(self, pre, obj, f, x, rtol, max_iters):
        """x (in: the guess, out: the solution) and f are flat float64 device tensors of one corrector's size; returns (iterations, relres)"""
        it, rel = C.c_int(0), C.c_double(0.0)
        self._cp_check(pre, "solve_rhs", obj, self.ptr(f), self.ptr(x), float(rtol), int(max_iters), C.byref(it), C.byref(rel))
        return it.value, rel.value

    def _cp_set_correctors(self, pre, obj, chi):
        self._cp_check(pre, "set_correctors", obj, self.ptr(chi))

    def _cp_correctors(self, pre, obj):
        nc, K, nn = self._cp_sizes(pre)
        return self._cp_device(pre, "correctors", K * nc * nn, obj)

    def _cp_energy_cells(self, pre, obj, p, q):
        return self._cp_device(pre, "energy_cells", self._cp_sizes(pre)[2], obj, int(p), int(q))

    def _cp_tensor(self, pre, obj):
        K = self._cp_sizes(pre)[1]
        out = np.zeros((K, K), dtype=np.float64)
        self._cp_check(pre, "tensor", obj, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def _cp_sensitivity(self, pre, obj, W, g):
        W = np.ascontiguousarray(W, dtype=np.float64)
        self._cp_check(pre, "sensitivity", obj, W.ctypes.data_as(C.POINTER(C.c_double)), self.ptr(g))

    def _cp_destroy(self, pre, obj):
        getattr(self.lib, f"lsm_{pre}_destroy")(obj)

    def homog_stiffness(self, obj, level):
        R = (1 << self.ndim) * self.ndim
        out = np.zeros((R, R), dtype=np.float64)
        self._cp_check("homog", "stiffness", obj, int(level), out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def homog_corrector(self, obj, k, u):
        self._cp_check("homog", "corrector", obj, int(k), *self._u3(u))

    def hcond_corrector(self, obj, k, u):
        self._cp_check("hcond", "corrector", obj, int(k), self.ptr(u))

    # ---- stress recovery (lsm_elastic_stress_*): `what` is L.STRESS_STRAIN, L.STRESS_STRESS or L.STRESS_VON_MISES
    def elastic_stress_cells(self, obj, u, what):
        """the component-major fp64 cell arrays as one flat device tensor"""
        N = self.ndim
        ncomp = 1 if what == L.STRESS_VON_MISES else N * (N + 1) // 2
        out = self.torch.empty(ncomp * int(np.prod([m - 1 for m in self.local_shape()])), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_stress_cells(obj, *self._u3(u), int(what), self.ptr(out)), "lsm_elastic_stress_cells")
        return out

    def elastic_stress(self, obj, u, what, outs):
        o = [self.ptr(t) for t in outs] + [None] * (6 - len(outs))
        L.check(self.h, self.lib.lsm_elastic_stress(obj, *self._u3(u), int(what), *o), "lsm_elastic_stress")

    def elastic_stress_norm(self, obj, u, p, sref):
        """(J′, smax)"""
        out = (C.c_double * 2)()
        L.check(self.h, self.lib.lsm_elastic_stress_norm(obj, *self._u3(u), float(p), float(sref), out), "lsm_elastic_stress_norm")
        return out[0], out[1]

    def elastic_stress_load(self, obj, u, p, sref):
        out = self.torch.empty(self.ndim * int(np.prod(self.local_shape())), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_stress_load(obj, *self._u3(u), float(p), float(sref), self.ptr(out)), "lsm_elastic_stress_load")
        return out

    def elastic_stress_sensitivity(self, obj, u, adj, p, sref, scale, g):
        L.check(self.h, self.lib.lsm_elastic_stress_sensitivity(obj, *self._u3(u), *self._u3(adj), float(p), float(sref), float(scale), self.ptr(g)),
                "lsm_elastic_stress_sensitivity")

    # ---- topological derivative of the compliance (lsm_elastic_topo*)
    def elastic_topo_cells(self, obj, u):
        """the fp64 cell array T_C as a flat device tensor"""
        out = self.torch.empty(int(np.prod([m - 1 for m in self.local_shape()])), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_topo_cells(obj, *self._u3(u), self.ptr(out)), "lsm_elastic_topo_cells")
        return out

    def elastic_topo(self, obj, u, out):
        L.check(self.h, self.lib.lsm_elastic_topo(obj, *self._u3(u), self.ptr(out)), "lsm_elastic_topo")

    # ---- thermoelastic coupling (lsm_elastic_thermal_*): T a padded field; alpha a float, or a flat float64 device tensor over the cells
    def _alpha(self, alpha):
        """(the scalar, the cell array's pointer)"""
        return (0.0, self.ptr(alpha)) if self.torch.is_tensor(alpha) else (float(alpha), None)

    def elastic_thermal_load(self, obj, T, t_ref, alpha):
        out = self.torch.empty(self.ndim * int(np.prod(self.local_shape())), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_thermal_load(obj, self.ptr(T), float(t_ref), *self._alpha(alpha), self.ptr(out)), "lsm_elastic_thermal_load")
        return out

    def elastic_thermal_stress_cells(self, obj, u, T, t_ref, alpha, what):
        """the component-major fp64 cell arrays as one flat device tensor"""
        N = self.ndim
        ncomp = 1 if what == L.STRESS_VON_MISES else N * (N + 1) // 2
        out = self.torch.empty(ncomp * int(np.prod([m - 1 for m in self.local_shape()])), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_thermal_stress_cells(obj, *self._u3(u), self.ptr(T), float(t_ref), *self._alpha(alpha), int(what), self.ptr(out)),
                "lsm_elastic_thermal_stress_cells")
        return out

    def elastic_thermal_stress(self, obj, u, T, t_ref, alpha, what, outs):
        o = [self.ptr(t) for t in outs] + [None] * (6 - len(outs))
        L.check(self.h, self.lib.lsm_elastic_thermal_stress(obj, *self._u3(u), self.ptr(T), float(t_ref), *self._alpha(alpha), int(what), *o),
                "lsm_elastic_thermal_stress")

    def elastic_thermal_source(self, obj, v, alpha):
        out = self.torch.empty(int(np.prod(self.local_shape())), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_thermal_source(obj, *self._u3(v), *self._alpha(alpha), self.ptr(out)), "lsm_elastic_thermal_source")
        return out

    def elastic_thermal_sensitivity(self, obj, u, v, T, t_ref, alpha, minus, g):
        L.check(self.h, self.lib.lsm_elastic_thermal_sensitivity(obj, *self._u3(u), *self._u3(v), self.ptr(T), float(t_ref), *self._alpha(alpha),
                                                                 None if minus is None else self.ptr(minus), self.ptr(g)), "lsm_elastic_thermal_sensitivity")

    # ---- vibration modes (lsm_elastic_modes_*): the modes object borrows the elastic object
    def modes_create(self, obj, phi, level, rho_in, rho_out, rho_cells, m):
        out = C.c_void_p()
        L.check(self.h, self.lib.lsm_elastic_modes_create(obj, self.ptr(phi), float(level), float(rho_in), float(rho_out), self.ptr(rho_cells), int(m),
                                                          C.byref(out)), "lsm_elastic_modes_create")
        return out

    def modes_mass(self, md):
        out = self.torch.empty(int(np.prod(self.local_shape())), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_modes_mass(md, self.ptr(out)), "lsm_elastic_modes_mass")
        return out

    def modes_solve(self, md, m, x0, rtol, max_iters):
        """returns (status, λ, relres, iterations, stats); status is OK or ERR_NOT_CONVERGED (whose message lsm_last_error keeps), anything else raises"""
        lam, rel, it, stats = (C.c_double * m)(), (C.c_double * m)(), C.c_int(0), (C.c_int64 * 4)()
        code = self.lib.lsm_elastic_modes_solve(md, self.ptr(x0), float(rtol), int(max_iters), lam, rel, C.byref(it), stats)
        if code != L.ERR_NOT_CONVERGED:
            L.check(self.h, code, "lsm_elastic_modes_solve")
        return code, np.array(lam[:]), np.array(rel[:]), it.value, tuple(int(v) for v in stats)

    def modes_vectors(self, md, count):
        out = self.torch.empty(int(count), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elastic_modes_vectors(md, self.ptr(out)), "lsm_elastic_modes_vectors")
        return out

    def modes_store(self, md, k, u):
        L.check(self.h, self.lib.lsm_elastic_modes_store(md, int(k), *self._u3(u)), "lsm_elastic_modes_store")

    def modes_sensitivity(self, md, k, g):
        L.check(self.h, self.lib.lsm_elastic_modes_sensitivity(md, int(k), self.ptr(g)), "lsm_elastic_modes_sensitivity")

    def modes_destroy(self, md):
        self.lib.lsm_elastic_modes_destroy(md)

    # ---- scalar eigenmodes (lsm_elliptic_modes_*): the modes object borrows the elliptic object
    def emodes_create(self, obj, phi, level, rho_in, rho_out, rho_cells, m):
        out = C.c_void_p()
        L.check(self.h, self.lib.lsm_elliptic_modes_create(obj, self.ptr(phi), float(level), float(rho_in), float(rho_out), self.ptr(rho_cells), int(m),
                                                           C.byref(out)), "lsm_elliptic_modes_create")
        return out

    def emodes_mass(self, md):
        out = self.torch.empty(int(np.prod(self.local_shape())), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elliptic_modes_mass(md, self.ptr(out)), "lsm_elliptic_modes_mass")
        return out

    def emodes_apply(self, md, ncols, x):
        """the block apply: x holds ncols columns of nn float64 values, zero on the fixed nodes; returns A x, the fixed rows zero"""
        y = self.torch.empty_like(x)
        L.check(self.h, self.lib.lsm_elliptic_modes_apply(md, int(ncols), self.ptr(x), self.ptr(y)), "lsm_elliptic_modes_apply")
        return y

    def emodes_solve(self, md, m, x0, rtol, max_iters):
        """returns (status, λ, relres, iterations, stats); status is OK or ERR_NOT_CONVERGED (whose message lsm_last_error keeps), anything else raises"""
        lam, rel, it, stats = (C.c_double * m)(), (C.c_double * m)(), C.c_int(0), (C.c_int64 * 4)()
        code = self.lib.lsm_elliptic_modes_solve(md, self.ptr(x0), float(rtol), int(max_iters), lam, rel, C.byref(it), stats)
        if code != L.ERR_NOT_CONVERGED:
            L.check(self.h, code, "lsm_elliptic_modes_solve")
        return code, np.array(lam[:]), np.array(rel[:]), it.value, tuple(int(v) for v in stats)

    def emodes_vectors(self, md, count):
        out = self.torch.empty(int(count), dtype=self.torch.float64, device=self.device)
        L.check(self.h, self.lib.lsm_elliptic_modes_vectors(md, self.ptr(out)), "lsm_elliptic_modes_vectors")
        return out

    def emodes_store(self, md, k, u):
        L.check(self.h, self.lib.lsm_elliptic_modes_store(md, int(k), self.ptr(u)), "lsm_elliptic_modes_store")

    def emodes_sensitivity(self, md, k, g):
        L.check(self.h, self.lib.lsm_elliptic_modes_sensitivity(md, int(k), self.ptr(g)), "lsm_elliptic_modes_sensitivity")

    def emodes_destroy(self, md):
        self.lib.lsm_elliptic_modes_destroy(md)

    # ---- pictures (lsm_render_*)
    def render_create(self, phi, mask, level):
        """the renderer of a field: builds the brick table; borrows phi and mask"""
        if getattr(self, "slab", None) is not None:
            raise L.LsmError("render_create: this backend holds a slab of a decomposed grid; lsm_render_create works on the whole grid of one device")
        out = C.c_void_p()
        L.check(self.h, self.lib.lsm_render_create(self.h, self.ptr(phi), self.ptr(mask), float(level), C.byref(out)), "lsm_render_create")
        return out

    def render_refresh(self, r):
        L.check(self.h, self.lib.lsm_render_refresh(r), "lsm_render_refresh")

    def render_draw(self, r, camera, width, height, style, want_normal=True):
        """one picture as device tensors: (rgba (H, W, 4) uint8, depth (H, W) float64 or cls (H, W) uint8, normal (H, W, 3) or None)"""
        t = self.torch
        W, H = int(width), int(height)
        if W <= 0 or H <= 0:
            raise L.LsmError("render_draw: width and height must be positive")
        three = self.ndim == 3
        rgba = t.empty((H, W, 4), dtype=t.uint8, device=self.device)
        aux = t.empty((H, W), dtype=t.float64 if three else t.uint8, device=self.device)
        normal = t.empty((H, W, 3), dtype=t.float64, device=self.device) if three and want_normal else None
        cam = None if camera is None else (C.c_double * 13)(*[float(x) for x in camera])
        sty = (C.c_double * len(style))(*[float(x) for x in style])
        L.check(self.h, self.lib.lsm_render_draw(r, cam, W, H, sty, self.ptr(rgba), self.ptr(aux), self.ptr(normal), None), "lsm_render_draw")
        return rgba, aux, normal

    def render_bricks(self, r):
        """the brick table (nb0, nb1, nb2) uint8 on the host: bits 0..1 state, bit 2 uniform"""
        t = self.torch
        dims = (C.c_int64 * 3)()
        L.check(self.h, self.lib.lsm_render_bricks(r, dims, None), "lsm_render_bricks")
        nb = tuple(int(d) for d in dims)
        tab = t.empty(max(nb[0] * nb[1] * nb[2], 1), dtype=t.uint8, device=self.device)
        L.check(self.h, self.lib.lsm_render_bricks(r, dims, self.ptr(tab)), "lsm_render_bricks")
        return tab.cpu().numpy()[:nb[0] * nb[1] * nb[2]].reshape(nb, order="F")

    def render_destroy(self, r):
        self.lib.lsm_render_destroy(r)

    # ---- meshes of the interior (lsm_vol_*)
    def vol_create(self, phi, mask, level):
        """returns (result handle, (vertices, elements, interface elements)); a band's mask is refused by the library"""
        if not self.torch.is_tensor(phi) or not phi.is_cuda:
            raise TypeError(f"vol_create takes a device buffer of this backend, not {type(phi).__name__}")
        if self.slab is not None:     # a one-rank group's slab is the whole grid with no communicator: the library could not tell
            raise L.LsmError("vol_create: this backend holds a slab of a decomposed grid; lsm_vol_create works on the whole grid of one device")
        out, cnt = C.c_void_p(), (C.c_int64 * 3)()
        L.check(self.h, self.lib.lsm_vol_create(self.h, self.ptr(phi), self.ptr(mask), float(level), C.byref(out), cnt), "lsm_vol_create")
        return out, tuple(int(v) for v in cnt)

    def vol_read(self, vol, counts):
        """the result's device arrays: vertices (nv, N) float64, elements (ne, N + 1) int64, interface (ni, N) int64"""
        t, N = self.torch, self.ndim
        nv, ne, ni = counts
        verts = t.empty((nv, N), dtype=t.float64, device=self.device)
        elems = t.empty((ne, N + 1), dtype=t.int64, device=self.device)
        iface = t.empty((ni, N), dtype=t.int64, device=self.device)
        L.check(self.h, self.lib.lsm_vol_read(vol, self.ptr(verts), self.ptr(elems), self.ptr(iface)), "lsm_vol_read")
        return verts, elems, iface

    def vol_destroy(self, vol):
        self.lib.lsm_vol_destroy(vol)

    def extend_along_normals(self, F, phi, frozen, nb_iters, cfl, interface_band, min_norm):
        work = [self.alloc()] + [self.alloc_side() for _ in range(self.ndim)]   # F staging + the normal components
        w = [self.ptr(x) for x in work] + [None] * (4 - len(work))
        L.check(self.h, self.lib.lsm_extend_along_normals(self.h, self.ptr(F), self.ptr(phi), self.ptr(frozen), w[0], w[1], w[2], w[3],
                                                          nb_iters, cfl, interface_band, min_norm), "lsm_extend_along_normals")
        self.sync()   # the work buffers are released on return

    # ---- narrow band (byte masks over the padded index space)
    def alloc_mask(self):
        return self.torch.zeros(int(self.lay.total), dtype=self.torch.uint8, device=self.device)

    def band_tile_count(self, mc):
        n = C.c_int64()
        L.check(self.h, self.lib.lsm_band_tile_count(self.h, int(mc), C.byref(n)), "lsm_band_tile_count")
        return int(n.value)

    def alloc_tiles(self, mc):
        return self.torch.zeros(self.band_tile_count(mc), dtype=self.torch.uint8, device=self.device)

    def alloc_halo_list(self, cap):
        """(entries, counter): 16-byte (node, nearest band node) records and the device uint32 count."""
        return (self.torch.empty(2 * int(cap), dtype=self.torch.int64, device=self.device),
                self.torch.zeros(1, dtype=self.torch.int32, device=self.device))

    def band_update(self, vals, mask, from_dense, nlayers, scratch_a, scratch_b, halo, tiles, mc, hlist, hcount):
        L.check(self.h, self.lib.lsm_band_update(self.h, self.ptr(vals), self.ptr(mask), 1 if from_dense else 0, int(nlayers),
                                                 self.ptr(scratch_a), self.ptr(scratch_b), self.ptr(halo), self.ptr(tiles), int(mc),
                                                 self.ptr(hlist), hlist.numel() // 2, self.ptr(hcount)), "lsm_band_update")

    def band_halo(self, vals, mask, halo, tiles, mc, hlist, hcount):
        L.check(self.h, self.lib.lsm_band_halo(self.h, self.ptr(vals), self.ptr(mask), self.ptr(halo), self.ptr(tiles), int(mc),
                                               self.ptr(hlist), hlist.numel() // 2, self.ptr(hcount)), "lsm_band_halo")

    def set_tuning(self, name, value):
        """lsm_set_tuning: one of the switches of include/lsm.h ("LSM_BAND_BRICKS", ...) on this handle."""
        L.check(self.h, self.lib.lsm_set_tuning(self.h, name.encode(), int(value)), "lsm_set_tuning")

    def get_tuning(self, name):
        v = C.c_int()
        L.check(self.h, self.lib.lsm_get_tuning(self.h, name.encode(), C.byref(v)), "lsm_get_tuning")
        return int(v.value)

    def band_retile(self, mask, tiles, mc):
        L.check(self.h, self.lib.lsm_band_retile(self.h, self.ptr(mask), self.ptr(tiles), int(mc)), "lsm_band_retile")

    def band_fill_list(self, vals, mask, hlist, hcount):
        L.check(self.h, self.lib.lsm_band_fill_list(self.h, self.ptr(vals), self.ptr(mask), self.ptr(hlist), hlist.numel() // 2,
                                                    self.ptr(hcount)), "lsm_band_fill_list")

    def band_prepare(self, vals, mask, hlist, hcount, tiles, mc):
        L.check(self.h, self.lib.lsm_band_prepare(self.h, self.ptr(vals), self.ptr(mask), self.ptr(hlist), hlist.numel() // 2,
                                                  self.ptr(hcount), self.ptr(tiles), int(mc)), "lsm_band_prepare")

    def band_status(self, hcount):
        n, m = C.c_int64(), C.c_int()
        L.check(self.h, self.lib.lsm_band_status(self.h, self.ptr(hcount), C.byref(n), C.byref(m)), "lsm_band_status")
        return int(n.value), bool(m.value)

    def band_fill(self, vals, mask, targets, tiles, mc):
        L.check(self.h, self.lib.lsm_band_fill(self.h, self.ptr(vals), self.ptr(mask), self.ptr(targets), self.ptr(tiles), int(mc)),
                "lsm_band_fill")

    def band_count(self, mask):
        n = C.c_int64()
        L.check(self.h, self.lib.lsm_band_count(self.h, self.ptr(mask), C.byref(n)), "lsm_band_count")
        return int(n.value)

    def band_missed(self):
        m = C.c_int()
        L.check(self.h, self.lib.lsm_band_missed(self.h, C.byref(m)), "lsm_band_missed")
        return bool(m.value)

    def stage_band(self, terms_c, nterms, psi, phin, out, out2, base_mode, cdt, cdt2, t, mask, tiles, mc):
        L.check(self.h, self.lib.lsm_stage_band(self.h, terms_c, nterms, self.ptr(psi), self.ptr(phin), self.ptr(out), self.ptr(out2),
                                                base_mode, cdt, cdt2, t, self.ptr(mask), self.ptr(tiles), int(mc), None), "lsm_stage_band")

    def band_c(self, mask, tiles, mc, hlist, hcount):
        """LsmBand: what lsm_band_update maintains for a field, as lsm_advance_band_* takes it."""
        return L.LsmBand(self.ptr(mask), self.ptr(tiles), int(mc), 0, self.ptr(hlist), hlist.numel() // 2, self.ptr(hcount))

    def advance_band(self, which, terms_c, nterms, band_c, phi, b1, b2, tc, dt, hook):
        cb = hook if hook is not None else C.cast(None, L.StageHook)
        if which == "fe":
            code = self.lib.lsm_advance_band_fe(self.h, terms_c, nterms, C.byref(band_c), self.ptr(phi), self.ptr(b1), tc, dt, cb, None)
        elif which == "rk2":
            code = self.lib.lsm_advance_band_rk2(self.h, terms_c, nterms, C.byref(band_c), self.ptr(phi), self.ptr(b1), self.ptr(b2), tc, dt, cb, None)
        else:
            code = self.lib.lsm_advance_band_rk3(self.h, terms_c, nterms, C.byref(band_c), self.ptr(phi), self.ptr(b1), self.ptr(b2), tc, dt, cb, None)
        L.check(self.h, code, f"lsm_advance_band_{which}")

    def compute_cfl_band(self, terms_c, nterms, phi, mask, t, tiles=None, mc=0):
        dt = C.c_double(0.0)
        L.check(self.h, self.lib.lsm_compute_cfl_band(self.h, terms_c, nterms, self.ptr(phi), self.ptr(mask), self.ptr(tiles), int(mc),
                                                      t, C.byref(dt)), "lsm_compute_cfl_band")
        return dt.value

    def mask_to_host(self, mask):
        """Boolean (local) interior of a mask, Fortran order."""
        flat = mask.cpu().numpy()
        n = tuple(int(self.lay.n[d]) for d in range(self.ndim))
        strides = tuple(int(self.lay.stride[d]) * flat.itemsize for d in range(self.ndim))   # the library's layout: pitch and origin are its own
        return np.lib.stride_tricks.as_strided(flat[int(self.lay.origin):], shape=n, strides=strides).astype(bool)

    def volume_local(self, t):
        out = C.c_double()
        L.check(self.h, self.lib.lsm_volume(self.h, self.ptr(t), C.byref(out)), "lsm_volume")
        return out.value

    def perimeter_local(self, t):
        out = C.c_double()
        L.check(self.h, self.lib.lsm_perimeter(self.h, self.ptr(t), C.byref(out)), "lsm_perimeter")
        return out.value

    def band_volume(self, t, mask):
        out = C.c_double()
        L.check(self.h, self.lib.lsm_band_volume(self.h, self.ptr(t), self.ptr(mask), C.byref(out)), "lsm_band_volume")
        return out.value

    def band_perimeter(self, t, mask):
        out = C.c_double()
        L.check(self.h, self.lib.lsm_band_perimeter(self.h, self.ptr(t), self.ptr(mask), C.byref(out)), "lsm_band_perimeter")
        return out.value

    def reinitialize(self, phi, mask, order, upsample, maxiters, xtol, ftol):
        work = self.alloc()
        nc, nfail, nfar = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.h, self.lib.lsm_reinitialize(self.h, self.ptr(phi), self.ptr(mask), self.ptr(work), int(order), int(upsample),
                                                  int(maxiters), float(xtol), float(ftol), C.byref(nc), C.byref(nfail), C.byref(nfar)),
                "lsm_reinitialize")
        return int(nc.value), int(nfail.value), int(nfar.value)

    def sync(self):
        L.check(self.h, self.lib.lsm_sync(self.h), "lsm_sync")

    def profile_enable(self, on=True):
        """on = True / 1: time every stage launch; N > 1: every N-th (lsm_profile_read scales); False / 0: off."""
        L.check(self.h, self.lib.lsm_profile_enable(self.h, int(on)), "lsm_profile_enable")

    def profile_read(self):
        n, ms = C.c_int64(), C.c_double()
        L.check(self.h, self.lib.lsm_profile_read(self.h, C.byref(n), C.byref(ms)), "lsm_profile_read")
        return n.value, ms.value


for _pre in ("homog", "hcond"):
    for _name in ("create", "cells", "apply", "load", "solve", "solve_rhs", "set_correctors", "correctors", "energy_cells", "tensor", "sensitivity", "destroy"):
        setattr(HipBackend, f"{_pre}_{_name}", functools.partialmethod(getattr(HipBackend, f"_cp_{_name}"), _pre))
