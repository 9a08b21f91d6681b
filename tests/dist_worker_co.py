"""One rank of tests/test_dist_gpu_co_gmres.py (launched by torch.distributed.run): the gpu
mode of tests/dist_worker.py with the stats of compressed-operator GMRES in the result --
``op_stats`` (Handle.gmres_operator_stats), ``basis_stats``, this rank's low product
``Av_low`` of a global random vector next to the fp64 ``Av``, and the layouts' bytes."""
import argparse
import json
import os

import numpy as np

import dist_worker as W  # (puts the repository and the package on sys.path)


def run_gpu(case, comm):
    import lib._native as N
    from lib.handle import Handle, params_to_options
    from oracle import synthetic as S
    from oracle.dist import local_rows
    N.check(N.lib().pls_set_device(0))
    spec = S.SynthSpec(case["dim"], case["N"])
    opts = dict(case["db"])
    opts.update(params_to_options(case["params"]))
    h = Handle.synthetic_dist(spec.dim, spec.N, spec.seed, spec.delta, opts, comm)
    rows = local_rows(spec.sizes(), comm.size, comm.rank)
    assert h.n == rows.size, (h.n, rows.size)
    b = S.rhs(spec)[rows]
    v = np.random.default_rng(5).standard_normal(spec.n)
    Av = h.matmult(v[rows])
    Av_low = h.matmult_single(v[rows])
    x, r = h.solve(b)
    out = dict(x=x, rows=rows, its=r.its, reason=r.reason, hist=h.history(), b=b, v=v, Av=Av, Av_low=Av_low,
               op_stats=np.array(h.gmres_operator_stats("global_")),
               basis_stats=np.array(h.gmres_basis_stats("global_")),
               layout=np.array(h.spmv_layout(), dtype=np.int64),
               layout_single=np.array(h.spmv_layout_single(), dtype=np.int64))
    h.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch.distributed as td
    td.init_process_group("gloo")
    from lib.dist import Communicator
    comm = Communicator.gloo()
    r = td.get_rank()
    for case in json.load(open(a.cases)):
        np.savez(os.path.join(a.out, f"{case['name']}_rank{r}.npz"), **run_gpu(case, comm))
    td.barrier()
    comm.destroy()
    td.destroy_process_group()


if __name__ == "__main__":
    main()
