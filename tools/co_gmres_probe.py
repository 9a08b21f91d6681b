"""Measurements for compressed-operator GMRES on bench.py's flagship
system (3-D synthetic, 2-way block PC, BJACOBI(ILU(0)) blocks): one JSON line per run.

  --mode rates   pls_bench_spmv against pls_bench_spmv_single (the fp32-value kernel at the depth
                 given by --depth, option pls.d16_unroll_single): seconds per launch, the bytes
                 each streams (matrix layout + x + y) and GB/s
  --mode solve   one warm-up and --steps timed solves with --variant double | basis | operator
                 (nothing, global_pls_gmres_basis single, that plus global_pls_gmres_operator
                 single): ms per solve, its, reason, the last history entry, gmres_operator_stats,
                 gmres_basis_stats, reuse_stats, SpMV time per call, device memory held
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "poroelasticity-linear-solvers_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402  (the flagship configuration's options)


def held_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        return None
    return total.value - free.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["rates", "solve"])
    ap.add_argument("--N", type=int, default=59)
    ap.add_argument("--variant", default="operator", choices=["double", "basis", "operator"])
    ap.add_argument("--depth", type=int, default=0, help="pls.d16_unroll_single (0: the default)")
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--opt", action="append", default=[])
    a = ap.parse_args()

    import lib._native as Nat
    from lib.handle import Handle, params_to_options
    Nat.check(Nat.lib().pls_set_device(0))
    args = argparse.Namespace(pc_type="diagonal", preset=None, inexact=False, solver="gmres", atol=1e-8, maxit=a.maxit,
                              inner="bjacobi", aar_order=10, blocks_s=256, blocks_fp=264, blocks_p=11)
    params, db = bench.solver_options(args)
    opts = dict(db)
    opts.update(params_to_options(params))
    opts["global_ksp_rtol"] = repr(a.rtol)
    if a.variant in ("basis", "operator"):
        opts["global_pls_gmres_basis"] = "single"
    if a.variant == "operator":
        opts["global_pls_gmres_operator"] = "single"
    if a.depth:
        opts["pls.d16_unroll_single"] = str(a.depth)
    for kv in a.opt:
        k, _, v = kv.partition("=")
        opts[k] = v
    h = Handle.synthetic(3, a.N, bench.SEED, bench.DELTA, opts)
    n = h.n
    d_b, d_x = Nat.DeviceArray(n), Nat.DeviceArray(n)
    h.rhs_device(bench.RHS_SEED, d_b.p)
    out = {"mode": a.mode, "N": a.N, "n": n, "nnz": h.nnz_A, "depth": a.depth or "default"}
    if a.mode == "rates":
        (_, mb), (_, mb32) = h.spmv_layout(), h.spmv_layout_single()
        h.bench_spmv(d_b.p, d_x.p, 3)
        h.bench_spmv_single(d_b.p, d_x.p, 3)
        t64 = h.bench_spmv(d_b.p, d_x.p, a.reps)
        t32 = h.bench_spmv_single(d_b.p, d_x.p, a.reps)
        b64, b32 = mb + 16.0 * n, mb32 + 16.0 * n
        out.update(sec_fp64=t64, sec_single=t32, bytes_fp64=b64, bytes_single=b32, gbs_fp64=b64 / t64 / 1e9,
                   gbs_single=b32 / t32 / 1e9, time_ratio=t32 / t64, bytes_ratio=b32 / b64)
    else:
        h.setup()
        h.create_solver()
        r = h.solve_device(d_b.p, d_x.p)
        h.reset_timings()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r = h.solve_device(d_b.p, d_x.p)
        dt = time.perf_counter() - t0
        tm = h.timings()
        hist = h.history()
        out.update(variant=a.variant, rtol=a.rtol, maxit=a.maxit, ms_per_solve=1e3 * dt / a.steps, its=r.its,
                   reason=r.reason, history_entries=int(hist.size), last_history_entry=float(hist[-1]),
                   operator_stats=h.gmres_operator_stats("global_"), basis_stats=h.gmres_basis_stats("global_"),
                   reuse_stats=h.reuse_stats(), spmv_ms_per_call=1e3 * tm["spmv_total"] / max(1, tm["spmv_calls"]),
                   spmv_calls_per_solve=tm["spmv_calls"] / a.steps, solver_ms=1e3 * tm["solver_total"] / a.steps,
                   held_bytes=held_bytes())
    print(json.dumps(out), flush=True)
    d_b.free()
    d_x.free()
    h.destroy()


if __name__ == "__main__":
    main()
