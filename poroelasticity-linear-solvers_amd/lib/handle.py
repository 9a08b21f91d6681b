"""Owning wrapper of a ``pls_handle`` (include/pls.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


def params_to_options(parameters: dict) -> dict:
    """The reference's parameter dict -> ``pls.*`` option keys."""
    keymap = {
        "solver type": "pls.solver_type", "solver atol": "pls.solver_atol", "solver rtol": "pls.solver_rtol",
        "solver maxiter": "pls.solver_maxiter", "solver monitor": "pls.solver_monitor",
        "pc type": "pls.pc_type", "inner ksp type": "pls.inner_ksp_type", "inner pc type": "pls.inner_pc_type",
        "inner rtol": "pls.inner_rtol", "inner atol": "pls.inner_atol", "inner maxiter": "pls.inner_maxiter",
        "inner monitor": "pls.inner_monitor", "inner accel order": "pls.inner_accel_order",
        "AAR order": "pls.aar_order", "AAR p": "pls.aar_p", "AAR omega": "pls.aar_omega", "AAR beta": "pls.aar_beta",
    }
    out = {}
    for k, v in parameters.items():
        if k in keymap:
            if isinstance(v, bool):
                v = "1" if v else "0"
            out[keymap[k]] = str(v).replace(" ", "_")
    return out


def options_text(d: dict) -> bytes:
    lines = []
    for k, v in d.items():
        lines.append(k if v is None else f"{k} {v}")
    return "\n".join(lines).encode()


class Handle:
    def __init__(self, ptr: C.c_void_p):
        self.ptr = ptr
        n, ns, nf, np_, nnz = (C.c_int64() for _ in range(5))
        N.check(N.lib().pls_get_sizes(ptr, C.byref(n), C.byref(ns), C.byref(nf), C.byref(np_), C.byref(nnz)))
        self.n, self.ns, self.nf, self.np, self.nnz_A = n.value, ns.value, nf.value, np_.value, nnz.value

    # ----------------------------------------------------------- creation --
    @classmethod
    def from_csr(cls, A, P, P_diff, is_s, is_f, is_p, bcs_sub_pressure, options: dict):
        keep = []

        def mk(M):
            if M is None:
                return None
            ai, aj, av, nr, nc = N.csr_of(M)
            keep.extend([ai, aj, av])
            return N.pls_csr(nr, nc, ai.ctypes.data, aj.ctypes.data, av.ctypes.data)

        cA, cP, cD = mk(A), mk(P), mk(P_diff)
        is_s, is_f, is_p = N.is_array(is_s), N.is_array(is_f), N.is_array(is_p)
        bcs = np.ascontiguousarray(np.asarray(bcs_sub_pressure if bcs_sub_pressure is not None else [],
                                              dtype=np.int32))
        out = C.c_void_p()
        N.check(N.lib().pls_create(C.byref(cA), C.byref(cP), C.byref(cD) if cD is not None else None,
                                   N.ptr(is_s), is_s.size, N.ptr(is_f), is_f.size, N.ptr(is_p), is_p.size,
                                   N.ptr(bcs), bcs.size, options_text(options), C.byref(out)))
        return cls(out)

    @classmethod
    def from_csr_dist(cls, A, P, P_diff, is_s, is_f, is_p, bcs_sub_pressure, options: dict, comm, row_start=None):
        """This rank's share of a caller-assembled system (pls_create_dist):
        A, P, P_diff = the rank's rows (global columns), is_* = the global
        indices of the dofs it owns, bcs_sub_pressure = positions inside its p
        sub-vector.  ``row_start`` (the rank's first global row) defaults to
        the smallest owned index.  Collective over ``comm``; host vectors are
        the rank's rows in the caller's order."""
        keep = []
        is_s, is_f, is_p = N.is_array(is_s), N.is_array(is_f), N.is_array(is_p)
        nloc = is_s.size + is_f.size + is_p.size
        if row_start is None:
            row_start = int(min(a.min() for a in (is_s, is_f, is_p) if a.size)) if nloc else 0

        def mk(M):
            if M is None:
                return None
            ai, aj, av, _, nc = N.csr_of(M)
            keep.extend([ai, aj, av])
            return N.pls_csr(ai.size - 1, nc, ai.ctypes.data, aj.ctypes.data, av.ctypes.data)

        cA, cP, cD = mk(A), mk(P), mk(P_diff)
        bcs = np.ascontiguousarray(np.asarray(bcs_sub_pressure if bcs_sub_pressure is not None else [],
                                              dtype=np.int32))
        out = C.c_void_p()
        N.check(N.lib().pls_create_dist(C.byref(cA), C.byref(cP), C.byref(cD) if cD is not None else None,
                                        int(row_start), N.ptr(is_s), is_s.size, N.ptr(is_f), is_f.size,
                                        N.ptr(is_p), is_p.size, N.ptr(bcs), bcs.size, options_text(options),
                                        comm.ptr, C.byref(out)))
        h = cls(out)
        h._comm = comm
        return h

    @classmethod
    def synthetic(cls, dim, Nel, seed, delta, options: dict):
        spec = N.pls_synth_spec(int(dim), int(Nel), int(seed), float(delta))
        out = C.c_void_p()
        N.check(N.lib().pls_create_synthetic(C.byref(spec), options_text(options), C.byref(out)))
        return cls(out)

    @classmethod
    def synthetic_dist(cls, dim, Nel, seed, delta, options: dict, comm):
        """This rank's share of the synthetic system on ``comm`` (lib/dist.py).

        Sizes and vectors are rank-local: [s_r | f_r | p_r] (PETSc row slabs)."""
        spec = N.pls_synth_spec(int(dim), int(Nel), int(seed), float(delta))
        out = C.c_void_p()
        N.check(N.lib().pls_create_synthetic_dist(C.byref(spec), options_text(options), comm.ptr, C.byref(out)))
        h = cls(out)
        h._comm = comm  # destroyed after the handle
        return h

    def update_matrices(self, A=None, P=None, P_diff=None):
        """New values / patterns for the next solves (pls_update_matrices); the
        block PC is set up again before the next solve."""
        keep = []

        def mk(M):
            if M is None:
                return None
            ai, aj, av, nr, nc = N.csr_of(M)
            keep.extend([ai, aj, av])
            return C.byref(N.pls_csr(nr, nc, ai.ctypes.data, aj.ctypes.data, av.ctypes.data))

        N.check(N.lib().pls_update_matrices(self.ptr, mk(A), mk(P), mk(P_diff)))

    # ------------------------------------------------------------- control --
    def set_option(self, key, value=None):
        N.check(N.lib().pls_set_option(self.ptr, str(key).encode(), None if value is None else str(value).encode()))

    def setup(self):
        N.check(N.lib().pls_setup(self.ptr))

    def create_solver(self):
        N.check(N.lib().pls_create_solver(self.ptr))

    def destroy(self):
        if self.ptr:
            N.lib().pls_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # --------------------------------------------------------- host vectors --
    def pc_apply(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        N.check(N.lib().pls_pc_apply(self.ptr, N.ptr(x), N.ptr(y)))
        return y

    def matmult(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        N.check(N.lib().pls_matmult(self.ptr, N.ptr(x), N.ptr(y)))
        return y

    def matmult_single(self, x):
        """y = A^ x: the outer operator with its stored values rounded to fp32 once, x and every sum
        fp64 (pls_matmult_single; what -<prefix>pls_gmres_operator single multiplies with)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        N.check(N.lib().pls_matmult_single(self.ptr, N.ptr(x), N.ptr(y)))
        return y

    def _guess_info(self, prefix):
        rx, t = C.c_int64(), C.c_double()
        N.check(N.lib().pls_get_ksp_guess_info(self.ptr, prefix.encode(), C.byref(rx), C.byref(t)))
        return bool(rx.value), t.value

    def initial_guess_nonzero(self):
        """Does the outer solve read x as its initial guess?  libpls's own answer
        (pls_get_ksp_guess_info; creates the solver if it was not yet)."""
        return self._guess_info("global_")[0]

    def solve(self, b, x0=None):
        """x, result = KSPSolve(b).  ``x0``: the initial guess, read by libpls exactly when
        -global_ksp_initial_guess_nonzero is set and no Fischer guess replaces it; passing one
        otherwise is an error, and without one the guess is zero."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        if x0 is not None:
            if not self.initial_guess_nonzero():
                raise ValueError("Handle.solve: x0 given, but global_ksp_initial_guess_nonzero is not set "
                                 "(or a Fischer guess replaces it): libpls would not read it")
            x = np.array(x0, dtype=np.float64, order="C", copy=True)
            if x.shape != b.shape:
                raise ValueError("Handle.solve: x0 must have the shape of b")
        else:
            x = np.zeros_like(b)  # (read as the guess when the option is set, never otherwise)
        r = N.pls_result()
        N.check(N.lib().pls_solve(self.ptr, N.ptr(b), N.ptr(x), C.byref(r)))
        return x, r

    # ------------------------------------------------------- device vectors --
    def solve_device(self, d_b, d_x):
        r = N.pls_result()
        N.check(N.lib().pls_solve_device(self.ptr, d_b, d_x, C.byref(r)))
        return r

    def pc_apply_device(self, d_x, d_y):
        N.check(N.lib().pls_pc_apply_device(self.ptr, d_x, d_y))

    def matmult_device(self, d_x, d_y):
        N.check(N.lib().pls_matmult_device(self.ptr, d_x, d_y))

    def matmult_single_device(self, d_x, d_y):
        N.check(N.lib().pls_matmult_single_device(self.ptr, d_x, d_y))

    def rhs_device(self, seed, d_b):
        N.check(N.lib().pls_synthetic_rhs_device(self.ptr, int(seed), d_b))

    def bench_spmv(self, d_x, d_y, reps):
        s = C.c_double()
        N.check(N.lib().pls_bench_spmv(self.ptr, d_x, d_y, int(reps), C.byref(s)))
        return s.value

    def bench_spmv_single(self, d_x, d_y, reps):
        s = C.c_double()
        N.check(N.lib().pls_bench_spmv_single(self.ptr, d_x, d_y, int(reps), C.byref(s)))
        return s.value

    def bench_global_sum(self, count, reps):
        s = C.c_double()
        N.check(N.lib().pls_bench_global_sum(self.ptr, int(count), int(reps), C.byref(s)))
        return s.value

    def spmv_layout(self):
        """(is SELL-64/D16, matrix bytes streamed per product of A)."""
        d, b = C.c_int32(), C.c_int64()
        N.check(N.lib().pls_spmv_layout(self.ptr, C.byref(d), C.byref(b)))
        return bool(d.value), b.value

    def spmv_layout_single(self):
        """(can A's layout carry the fp32 value stream, matrix bytes streamed per low product of A)."""
        d, b = C.c_int32(), C.c_int64()
        N.check(N.lib().pls_spmv_layout_single(self.ptr, C.byref(d), C.byref(b)))
        return bool(d.value), b.value

    # -------------------------------------------------------------- queries --
    def result(self):
        r = N.pls_result()
        N.check(N.lib().pls_get_result(self.ptr, C.byref(r)))
        return r

    def history(self):
        r = self.result()
        h = np.zeros(max(r.history_len, 1), dtype=np.float64)
        N.check(N.lib().pls_get_history(self.ptr, N.ptr(h), r.history_len))
        return h[:r.history_len]

    def timings(self):
        t = N.pls_timings()
        N.check(N.lib().pls_get_timings(self.ptr, C.byref(t)))
        return {f: getattr(t, f) for f, _ in t._fields_}

    def ksp_stats(self, prefix):
        """(solves, iterations, most iterations of one solve, solves with a negative reason,
        the most recent negative reason) of the inner solver with this options prefix
        (pls_get_ksp_stats)."""
        s = np.zeros(5, dtype=np.int64)
        N.check(N.lib().pls_get_ksp_stats(self.ptr, prefix.encode(), N.ptr(s)))
        return tuple(int(v) for v in s)

    def gmres_orthog_stats(self, prefix):
        """(Arnoldi steps orthogonalised, second classical Gram-Schmidt passes, scheme: 0 CGS
        refine_never, 1 refine_ifneeded, 2 refine_always, 3 modified Gram-Schmidt) of the gmres /
        fgmres solver with this options prefix (pls_get_gmres_orthog_stats)."""
        s = np.zeros(3, dtype=np.int64)
        N.check(N.lib().pls_get_gmres_orthog_stats(self.ptr, prefix.encode(), N.ptr(s)))
        return tuple(int(v) for v in s)

    def gmres_basis_stats(self, prefix):
        """(basis precision: 0 double, 1 single; bytes of the basis allocation; cycles ended by the
        drop rule; converged estimates confirmed against the true residual; confirmations that
        failed) of the gmres / fgmres solver with this options prefix (pls_get_gmres_basis_stats)."""
        s = np.zeros(5, dtype=np.int64)
        N.check(N.lib().pls_get_gmres_basis_stats(self.ptr, prefix.encode(), N.ptr(s)))
        return tuple(int(v) for v in s)

    def gmres_operator_stats(self, prefix):
        """(operator precision inside the Arnoldi step: 0 double, 1 single; bytes of the fp32 value
        streams held; low-precision products; fp64 products) of the gmres / fgmres solver with this
        options prefix (pls_get_gmres_operator_stats)."""
        s = np.zeros(4, dtype=np.int64)
        N.check(N.lib().pls_get_gmres_operator_stats(self.ptr, prefix.encode(), N.ptr(s)))
        return tuple(int(v) for v in s)

    def ksp_guess_stats(self, prefix):
        """((type: 0 none, 1 fischer; columns stored now; size; guesses formed; updates skipped;
        resets), ||b - A x0|| / ||b|| of the most recent guessed solve -- NaN before the first) of
        the KSP with this options prefix (pls_get_ksp_guess_stats)."""
        s = np.zeros(6, dtype=np.int64)
        red = C.c_double()
        N.check(N.lib().pls_get_ksp_guess_stats(self.ptr, prefix.encode(), N.ptr(s), C.byref(red)))
        return tuple(int(v) for v in s), red.value

    def ksp_guess_time(self, prefix):
        """Seconds (HIP events) the most recent solve of that KSP spent on its guess: x0, r0 and the
        norms before the zero-guess solve, x = x0 + d and the space's update after it; NaN unless
        pls.ksp_guess_timing 1 (pls_get_ksp_guess_info)."""
        return self._guess_info(prefix)[1]

    def chebyshev_bounds(self, prefix):
        """(emin, emax as used, the estimate's smallest and largest real part -- NaN when the bounds
        were given explicitly) of the chebyshev solver with this options prefix, after its first
        solve (pls_get_chebyshev_bounds)."""
        s = np.zeros(4, dtype=np.float64)
        N.check(N.lib().pls_get_chebyshev_bounds(self.ptr, prefix.encode(), N.ptr(s)))
        return tuple(float(v) for v in s)

    def ilu_fill(self, prefix):
        """(levels of fill, entries of the block-truncated matrix before the fill, after it, the
        longest filled row) of the ilu / bjacobi(ilu) PC with this options prefix (pls_get_ilu_fill)."""
        s = np.zeros(4, dtype=np.int64)
        N.check(N.lib().pls_get_ilu_fill(self.ptr, prefix.encode(), N.ptr(s)))
        return tuple(int(v) for v in s)

    def asm_stats(self, prefix):
        """(blocks, overlap, type as 0 restrict / 1 basic / 2 interpolate / 3 none, rows of all
        subdomains together, rows of the largest, 1 when the fused kernel serves the application)
        of the asm PC with this options prefix (pls_get_asm_stats)."""
        s = np.zeros(6, dtype=np.int64)
        N.check(N.lib().pls_get_asm_stats(self.ptr, prefix.encode(), N.ptr(s)))
        return tuple(int(v) for v in s)

    def asm_rows(self, prefix):
        """(ptr int64[blocks + 1], rows int32): the subdomains of the asm PC with this options
        prefix, each ascending, numbered within the prefix's block (pls_get_asm_rows)."""
        s = self.asm_stats(prefix)
        ptr = np.zeros(s[0] + 1, dtype=np.int64)
        rows = np.zeros(max(s[3], 1), dtype=np.int32)
        N.check(N.lib().pls_get_asm_rows(self.ptr, prefix.encode(), N.ptr(ptr), N.ptr(rows)))
        return ptr, rows[:s[3]]

    def boomeramg_relax(self, prefix):
        """(stats, lambda) of the BoomerAMG stand-in with this options prefix (pls_get_boomeramg_relax):
        stats = (relax type 0 symmetric-SOR/Jacobi / 1 Jacobi / 2 l1scaled-Jacobi / 3 Chebyshev,
        smoothed levels, Chebyshev order, levels on the fused step, fused step launches and
        elementwise step launches of the last application); lambda: the levels' eigenvalue
        estimates (0 for the other types).  Sets the preconditioner up if it was not yet."""
        s = np.zeros(6, dtype=np.int64)
        lam = np.zeros(32, dtype=np.float64)
        N.check(N.lib().pls_get_boomeramg_relax(self.ptr, prefix.encode(), N.ptr(s), N.ptr(lam), 32))
        return tuple(int(v) for v in s), lam[:int(s[1])].copy()

    def relax_step(self, m, b, x, d=None, a=0.0, g=1.0, fused=True):
        """One smoothing step on the outer operator A (pls_relax_step; a diagnostic):
        x_new = x + dn, dn = a d + g (m (b - A x)); d None: no a d term.  Returns
        (x_new, d_new or None, was_fused)."""
        m, b, x = (np.ascontiguousarray(v, dtype=np.float64) for v in (m, b, x))
        dn = None if d is None else np.array(d, dtype=np.float64)
        y = np.empty_like(x)
        wf = C.c_int32()
        N.check(N.lib().pls_relax_step(self.ptr, N.ptr(m), N.ptr(b), N.ptr(x), None if dn is None else N.ptr(dn),
                                       float(a), float(g), int(bool(fused)), N.ptr(y), C.byref(wf)))
        return y, dn, bool(wf.value)

    def bc_columns_stats(self, prefix):
        """(mode: 0 keep, 1 lift, 2 drop; constrained rows; entries moved to C; rows of C; bytes the
        KSP holds for K' and C) of the inner solver with this options prefix (<prefix>pls_bc_columns,
        pls_get_bc_columns_stats).  Sets the preconditioner up if it was not yet."""
        s = np.zeros(5, dtype=np.int64)
        N.check(N.lib().pls_get_bc_columns_stats(self.ptr, prefix.encode(), N.ptr(s)))
        return tuple(int(v) for v in s)

    def bc_columns_matrix(self, prefix):
        """(bc_rows int32, c_rp int64[n + 1], c_ci int32, c_val float64): the constrained rows of
        the block this prefix solves and the moved entries C as CSR over all its rows, numbered
        within the block (pls_get_bc_columns_matrix)."""
        sizes = {"s_": self.ns, "f_": self.nf, "p_": self.np, "diff_": self.np, "fp_": self.nf + self.np,
                 "fp_fieldsplit_0_": self.np, "fp_fieldsplit_1_": self.nf}
        if prefix not in sizes:
            raise ValueError(f"Handle.bc_columns_matrix: no inner solver with prefix {prefix!r}")
        s = self.bc_columns_stats(prefix)
        rows = np.zeros(max(s[1], 1), dtype=np.int32)
        rp = np.zeros(sizes[prefix] + 1, dtype=np.int64)
        ci = np.zeros(max(s[2], 1), dtype=np.int32)
        v = np.zeros(max(s[2], 1), dtype=np.float64)
        N.check(N.lib().pls_get_bc_columns_matrix(self.ptr, prefix.encode(), N.ptr(rows), N.ptr(rp), N.ptr(ci),
                                                  N.ptr(v)))
        return rows[:s[1]], rp, ci[:s[2]], v[:s[2]]

    def reuse_stats(self):
        """(reduced outer products, full outer products since the last reset_timings, eligible 0/1)
        of the coupling reuse (pls_get_reuse_stats)."""
        s = np.zeros(3, dtype=np.int64)
        N.check(N.lib().pls_get_reuse_stats(self.ptr, N.ptr(s)))
        return tuple(int(v) for v in s)

    def reuse_wide(self):
        """(reuse rows served by several lanes, their lanes per row, lane-per-row reuse rows, bytes
        one reduced outer product streams from its layout); zeros while the coupling reuse is not
        eligible (pls_get_reuse_wide, option pls.reuse_wide)."""
        s = np.zeros(4, dtype=np.int64)
        N.check(N.lib().pls_get_reuse_wide(self.ptr, N.ptr(s)))
        return tuple(int(v) for v in s)

    def d16_share(self, which=0):
        """(shared 0/1, slices, slices with fewer than 64 classes, stored deltas, layouts this handle
        built with a shared delta stream) of A's layout (which 0) or of the reduced outer layout
        (which 1) (pls_get_d16_share)."""
        s = np.zeros(5, dtype=np.int64)
        N.check(N.lib().pls_get_d16_share(self.ptr, int(which), N.ptr(s)))
        return tuple(int(v) for v in s)

    def reuse_rows(self):
        """uint8 mask, the caller's row order: 1 on the rows the reduced outer product starts from
        the block PC's raw sums; all 0 while the coupling reuse is not eligible (pls_get_reuse_rows)."""
        m = np.zeros(self.n, dtype=np.uint8)
        N.check(N.lib().pls_get_reuse_rows(self.ptr, N.ptr(m)))
        return m

    def reset_timings(self):
        N.check(N.lib().pls_reset_timings(self.ptr))

    def export_matrix(self, which=0):
        import scipy.sparse as sp
        nr, nnz = C.c_int64(), C.c_int64()
        N.check(N.lib().pls_export_matrix(self.ptr, which, C.byref(nr), C.byref(nnz), None, None, None))
        rp = np.zeros(nr.value + 1, dtype=np.int64)
        ci = np.zeros(nnz.value, dtype=np.int32)
        v = np.zeros(nnz.value, dtype=np.float64)
        N.check(N.lib().pls_export_matrix(self.ptr, which, C.byref(nr), C.byref(nnz), N.ptr(rp), N.ptr(ci), N.ptr(v)))
        return sp.csr_matrix((v, ci, rp), shape=(nr.value, nr.value))

    def permutation(self):
        p = np.zeros(self.n, dtype=np.int64)
        N.check(N.lib().pls_get_permutation(self.ptr, N.ptr(p)))
        return p


def boomeramg_host_level(A, options: dict, prefix: str, level: int):
    """Level ``level`` of the classical AMG hierarchy (-pc_type hypre) that
    libpls builds from ``A`` on the host (``pls_boomeramg_host_level``; no
    device needed): (nlevels, n, nc, cf int8[n], P scipy CSR); on the coarsest
    level cf is empty and P is the coarsest operator."""
    import scipy.sparse as sp
    ai, aj, av, nr, nc_ = N.csr_of(A)
    m = N.pls_csr(nr, nc_, ai.ctypes.data_as(C.c_void_p), aj.ctypes.data_as(C.c_void_p), av.ctypes.data_as(C.c_void_p))
    nl, n, nc, nnz = (C.c_int64() for _ in range(4))
    args = [C.byref(m), options_text(options), prefix.encode(), int(level), C.byref(nl), C.byref(n), C.byref(nc),
            C.byref(nnz)]
    N.check(N.lib().pls_boomeramg_host_level(*args, None, None, None, None))
    cf = np.zeros(n.value if level < nl.value - 1 else 0, dtype=np.int8)
    rp = np.zeros(n.value + 1, dtype=np.int64)
    ci = np.zeros(max(nnz.value, 1), dtype=np.int32)
    v = np.zeros(max(nnz.value, 1), dtype=np.float64)
    N.check(N.lib().pls_boomeramg_host_level(*args, cf.ctypes.data_as(C.c_void_p) if cf.size else None,
                                             rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                             v.ctypes.data_as(C.c_void_p)))
    ncols = nc.value if level < nl.value - 1 else n.value
    P = sp.csr_matrix((v[:nnz.value], ci[:nnz.value], rp), shape=(n.value, ncols))
    return nl.value, n.value, nc.value, cf, P


LU_STATS = ("n", "fronts", "levels", "max_front", "solve_doubles", "workspace_doubles", "flops", "order_s",
            "symbolic_s", "max_separator")


def sparse_lu_analyze(A, options: dict | None = None, tree: bool = False):
    """Ordering + symbolic analysis of the sparse LU libpls would build on the
    square matrix ``A`` (``pls_sparse_lu_analyze``; host only, no device):
    fronts, tree levels, largest front, doubles one solve reads, doubles
    stored, factorization flops, timings (keys: ``LU_STATS``).  With
    ``tree``: (stats, perm, front_of, parent) -- ND position -> row, position ->
    front (postorder numbers), the fronts' parents."""
    ai, aj, av, nr, nc_ = N.csr_of(A)
    m = N.pls_csr(nr, nc_, ai.ctypes.data_as(C.c_void_p), aj.ctypes.data_as(C.c_void_p), av.ctypes.data_as(C.c_void_p))
    out = (C.c_double * len(LU_STATS))()
    N.check(N.lib().pls_sparse_lu_analyze(C.byref(m), options_text(options or {}), out, len(LU_STATS), None, None,
                                          None))
    stats = dict(zip(LU_STATS, list(out)))
    if not tree:
        return stats
    perm, front_of = np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int32)
    parent = np.zeros(int(stats["fronts"]), dtype=np.int32)
    N.check(N.lib().pls_sparse_lu_analyze(C.byref(m), options_text(options or {}), out, len(LU_STATS),
                                          perm.ctypes.data_as(C.c_void_p), front_of.ctypes.data_as(C.c_void_p),
                                          parent.ctypes.data_as(C.c_void_p)))
    return stats, perm, front_of, parent
