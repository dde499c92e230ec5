"""Worker of tests/test_cma_starts.py::test_host_multi_start_over_gloo: one rank of a world_size-N gloo group on CPU running
CMAOptimizer.optimize(..., starts=3) over its shard of the points, as tests/_dist_cma_worker.py runs the single start: the
communicator calls of alproj_amd._lib go to gloo, and the point set's evaluation is the oracle on the shard + ONE all-reduce of
P + 1 doubles (alproj_amd.dist).  Test infrastructure: the product has no such path.
usage: _dist_cma_starts_worker.py RANK WORLD PORT OUT_NPZ
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    import pandas as pd
    import torch
    import torch.distributed as dist
    from alproj_amd import _lib
    from alproj_amd import dist as adist
    from alproj_amd import optimize as aopt
    from alproj_amd import synthetic as syn
    from oracle import ref_numpy as orc

    dist.init_process_group("gloo", rank=rank, world_size=world)
    log = []

    def comm_bcast(array, root=0):
        t = torch.from_numpy(array.reshape(-1).view(np.uint8))     # bytes, in place, like alp_comm_bcast
        dist.broadcast(t, src=root)
        log.append(("bcast", str(array.dtype), tuple(array.shape)))
        return array

    _lib.comm_info = lambda: (rank, world)
    _lib.comm_bcast = comm_bcast

    truth = syn.truth_params(316)
    init = dict(truth, pan=truth["pan"] + 1.5, tilt=truth["tilt"] - 1.0, fov=truth["fov"] + 2, x=truth["x"] + 3)
    n = 1201
    xyz = syn.gcp_points(n, truth, seed=11)
    uv = orc.project_points(xyz, truth) + np.random.default_rng(11).normal(0, 0.8, (n, 2))
    lo, hi = adist.shard_bounds(n, rank, world)

    class ShardPoints:
        """what alproj_amd._lib.Points is to the optimiser, on this rank's shard"""
        precision, n = _lib.ALP_F64, hi - lo

        def eval_population(self, cand, kind, f_scale, want_argmin=True):
            sums = np.empty(len(cand))
            for i, c in enumerate(cand):
                p = orc.vector_to_params(c)
                proj = orc.project_points(xyz[lo:hi], p)
                loss = orc.mean_distance(uv[lo:hi], proj) if kind == _lib.LOSS_MEAN_DIST else orc.huber(uv[lo:hi], proj, f_scale)
                sums[i] = loss * (hi - lo)
            t = torch.from_numpy(adist.pack_partials(sums, hi - lo))
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            log.append(("eval", len(cand)))
            return adist.combine_partials(t.numpy())

        def close(self):
            pass

    aopt.BaseOptimizer._device_points = lambda self, precision=None: ShardPoints()
    o = aopt.CMAOptimizer(pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"]), init)
    o.set_target(syn.TARGETS_D9)
    params, err = o.optimize(generation=15, sigma=0.3, population_size=12, f_scale=10.0, seed=None, progress=False, starts=3)
    keys = syn.TARGETS_D9
    np.savez(out, params=np.array([params[k] for k in keys]), err=err,
             seeds=np.array([s for s, _, _ in o.start_results], dtype=np.uint64),
             start_params=np.array([[p[k] for k in keys] for _, p, _ in o.start_results]),
             start_errors=np.array([e for _, _, e in o.start_results]), log=np.array([repr(e) for e in log]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
