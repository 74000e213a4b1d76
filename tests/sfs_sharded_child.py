"""One rank of tests/test_sfs_sharded_gpu.py::test_two_processes_one_gpu (a child process, not a test module): joins a gloo
group over loopback, takes its three faces of ref_sfs's (6, 5, 4) case and calls the objective's
spherical_harmonics_intensity on cuda:0 three ways; everything it computed goes into one .npz for the parent to judge.

    python sfs_sharded_child.py RANK WORLD PORT OUT.npz"""
import datetime
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_sfs as RS  # noqa: E402

SHAPE, PER_RANK, DEV = (6, 5, 4), 3, "cuda:0"


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    L = importlib.import_module("3dfacerecon_amd.nets.losses")
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))   # (a lone rank gives up instead of waiting)
    try:
        d, g = RS.inputs(*SHAPE), RS.grad_out(*SHAPE)
        lo, hi = rank * PER_RANK, (rank + 1) * PER_RANK
        t = {k: torch.as_tensor(np.ascontiguousarray(v[lo:hi]), device=DEV) for k, v in d.items()}
        gt = torch.as_tensor(np.ascontiguousarray(g[lo:hi]), device=DEV)
        res = {}

        def run(tag, **kw):
            n = t["normal"].clone().requires_grad_(True)
            n2 = t["normal_new"].clone().requires_grad_(True)
            I = L.spherical_harmonics_intensity(t["abedo"], n, t["im_gray"], t["abedo_new"], n2, **kw)
            I.backward(gt)
            res[tag + "_intensity"], res[tag + "_gn"], res[tag + "_gn2"] = (x.detach().cpu().numpy() for x in (I, n.grad, n2.grad))
        run("sharded", gather=True, fused=True, fused_gather=True, rcond=RS.RCOND)
        run("default", gather=True, fused=True, rcond=RS.RCOND)        # flag off: the torch route, as before
        run("torch", gather=True, rcond=RS.RCOND)                      # ... which is this call
        torch.cuda.synchronize()
        np.savez(out, **res)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
