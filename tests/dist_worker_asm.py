"""One rank of tests/test_dist_gpu_asm.py (launched by torch.distributed.run): a sharded handle
with ``s_pc_type asm`` is set up, and the refusal's message is the result (``error``; empty when
the setup went through)."""
import argparse
import json
import os

import numpy as np

import dist_worker as W  # noqa: F401  (puts the repository and the package on sys.path)


def run_gpu(case, comm):
    import lib._native as N
    from lib.handle import Handle, params_to_options
    from oracle import synthetic as S
    N.check(N.lib().pls_set_device(0))
    spec = S.SynthSpec(case["dim"], case["N"])
    opts = dict(case["db"])
    opts.update(params_to_options(case["params"]))
    h = Handle.synthetic_dist(spec.dim, spec.N, spec.seed, spec.delta, opts, comm)
    error = ""
    try:  # (every rank's s block has a halo, so every rank is refused at the same place)
        h.setup()
    except RuntimeError as e:
        error = str(e)
    h.destroy()
    return dict(error=np.array(error), size=comm.size)


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
