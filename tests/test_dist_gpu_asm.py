"""``s_pc_type asm`` on two ranks (sharing the box's one GPU through the host-staged
communicator) is refused when the solver is created: overlap across ranks is out of scope, and
the message names the key and the rank count."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_dist_gpu as T
from distutil import free_port

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_DB = dict(T.CASES[0]["db"], s_pc_type="asm", s_pc_asm_blocks="4")
CASES = [{"name": "asm_refused", "dim": 2, "N": 6, "db": _DB, "params": T.BASE}]


def _launch(cases, world, tmp, timeout=300):
    cf = os.path.join(tmp, "cases.json")
    with open(cf, "w") as f:
        json.dump(cases, f)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}",
           os.path.join(HERE, "dist_worker_asm.py"), "--cases", cf, "--out", tmp]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "2")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, f"ranks failed (rc={p.returncode}):\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return {c["name"]: [dict(np.load(os.path.join(tmp, f"{c['name']}_rank{r}.npz"))) for r in range(world)]
            for c in cases}


def test_asm_is_refused_on_two_ranks(tmp_path):
    parts = _launch(CASES, 2, str(tmp_path))["asm_refused"]
    assert len(parts) == 2
    for p in parts:
        msg = str(p["error"])
        print(msg)
        assert re.search(r"s_pc_type asm.*sharded over 2 ranks", msg), msg
