"""Worker for tests/test_incremental_recycling.py: one rank of a sharded tree solve whose tree has recycled and marginalized
cliques, on the CPU (gloo, oracle backend); the share of this rank is compiled by the native host."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import iif_amd_loader  # noqa: E402

iif = iif_amd_loader.load()
import incremental_cases as cases  # noqa: E402
from iif_amd import abi, bayestree, native_host  # noqa: E402
from iif_amd.dist_solver import ShardedRunner, choose_transport  # noqa: E402
from oracle.oracle_backend import OracleBackend  # noqa: E402


def build():
    """the 24-variable chain under nested dissection: every third clique recycled, one inner clique marginalized"""
    fg = cases.chain24()
    tree = iif.buildTreeReset(fg, iif.nestedDissectionOrder(fg))
    cases.mark_third_recycled(tree)
    k = next(k for k, c in tree.cliques.items() if c.children and c.parent >= 0 and c.status == bayestree.NULL)
    tree.cliques[k].status, tree.cliques[k].allmarginalized = bayestree.MARGINALIZED, True
    return fg, tree


class Share:
    """this rank's share from nbp_tree_set_owner / nbp_tree_schedule, in the shape ShardedRunner reads"""

    def __init__(self, fg, tree, world, rank, seed):
        g = native_host.NativeGraph.from_fg(fg)
        nt = g.build_tree(tree.eliminationOrder)
        nt.push_statuses(tree)
        self.owner = nt.partition(world)
        nt.set_owner(self.owner, rank)
        self.n_slots = nt.plan_slots(False)
        nt.schedule(seed)
        ctype = {abi.STAGE_PROPOSALS: abi.ProposalDesc, abi.STAGE_PRODUCTS: abi.ProductDesc, abi.STAGE_COPIES: abi.CopyDesc,
                 abi.STAGE_DECONV: abi.ProposalDesc, abi.STAGE_COPY_POINTS: abi.CopyDesc}
        self.stages = []
        for kind, raw in nt.stages():
            n = len(raw) // C.sizeof(ctype[kind])
            self.stages.append((kind, list((ctype[kind] * n).from_buffer_copy(raw)) if n else []))
        self.segments, self.main, self.stats = nt.segments(), nt.main, nt.stats()
        self.n_messages = self.stats["messages"]
        self.cliques = [k for k in range(1, nt.n_cliques + 1) if self.owner[k] == rank]
        self._keep = (g, nt)


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    fg, tree = build()
    tp = Share(fg, tree, world, rank, 7)
    be = OracleBackend(100, tp.n_slots, 0, threads=2)
    for v in fg.ls():
        var = fg.getVariable(v)
        be.slot_write(tp.main[v], var.varType.manifold, var.val, var.bw)
    stride = iif.abi.slot_stride(100)
    arena_t = torch.from_numpy(be.arena)
    transport, group = choose_transport(dist, "cpu")
    ShardedRunner(tp, be, dist, lambda s: arena_t[s * stride:(s + 1) * stride], transport=transport, group=group).run()
    res = {}
    for c in tp.cliques:
        for v in tree.cliques[c].frontalIDs:
            res[v], res[v + "_bw"] = be.slot_read(tp.main[v], fg.getVariable(v).varType.manifold)
    np.savez(out, updates_up=tp.stats["updates_up"], updates_down=tp.stats["updates_down"], **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
